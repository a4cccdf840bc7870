"""PPO's target_kl, the host side without a device: the three C symbols and the record's layout against the header's
text, the config field, the refusals that come before any device work, the sweep key, what a trainer asks of its MLP handle (on fakes), the
logger's early-stopping line and the epoch graph key."""
from __future__ import annotations

import ctypes as C
import io
import re
import types

import pytest
import torch

import abi
from rl_brain_trainer_amd import mlp as kmlp
from rl_brain_trainer_amd import monitor as kmon
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import population as kpop
from rl_brain_trainer_amd import ppo as kppo

SYMBOLS = {"kp1_mlp_set_kl_gate": 4, "kp1_mlp_kl_gate_arm": 2, "kp1_mlp_kl_gate_read": 4}
CTYPES = {"double": C.c_double, "int32_t": C.c_int32, "float": C.c_float}


def _header() -> str:
    return abi.header("kp1_ppo.h")


def test_symbols_declared_exported_and_bound():
    for name, n_args in SYMBOLS.items():
        assert len(abi.params(name, "kp1_ppo.h")) == n_args, name        # raises if include/kp1_ppo.h does not declare it
        assert name in native.declared_symbols()
    L = native.load()
    for name, n_args in SYMBOLS.items():
        assert hasattr(L, name), f"libkp1.so does not export {name}"
        assert len(getattr(L, name).argtypes) == n_args, name


def test_record_struct_matches_the_header():
    m = re.search(r"typedef\s+struct\s+kp1_kl_gate\s*\{(.*?)\}\s*kp1_kl_gate\s*;", _header(), flags=re.S)
    assert m, "kp1_kl_gate is not declared in include/kp1_ppo.h"
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), CTYPES[ctype]) for n in names.split(",")]
    rebuilt = type("Rebuilt", (C.Structure,), {"_fields_": fields})
    assert [f for f, _ in fields][:6] == ["threshold", "stopped", "n_counted", "n_seen", "stop_index", "stop_kl"]
    assert list(native.KlGate._fields_) == fields
    assert C.sizeof(native.KlGate) == C.sizeof(rebuilt) == 32
    for name, _ in fields:
        assert getattr(native.KlGate, name).offset == getattr(rebuilt, name).offset, name


def test_config_field():
    assert kppo.PPOConfig().target_kl is None
    assert list(kppo.PPOConfig.__dataclass_fields__)[-1] == "target_kl"      # last: positional use of the older fields is unchanged
    assert kppo.PPOConfig.from_algo_kwargs({"target_kl": 0.02}).target_kl == 0.02
    assert kppo.PPOConfig.from_algo_kwargs({"learning_rate": 1e-4}).target_kl is None
    with pytest.raises(TypeError, match="unexpected keyword"):
        kppo.PPOConfig.from_algo_kwargs({"target_kl_": 0.02})


def test_targets_without_a_value_are_none():
    assert kppo.check_target_kl([None, 0.0, -1.0, float("nan"), 0.03], kppo.Dist()) == [None, None, None, None, 0.03]


class _SetupReached(Exception):
    pass


def _no_setup(monkeypatch):
    def boom(self, *a, **k):
        raise _SetupReached()

    monkeypatch.setattr(kppo.PPO, "_setup", boom)


def _fake_env():
    return types.SimpleNamespace(dtype=torch.float32, is_population=False, device=torch.device("cpu"), n_envs=4)


def test_refused_under_data_parallel_before_setup(monkeypatch):
    _no_setup(monkeypatch)
    dist = types.SimpleNamespace(enabled=True, world_size=2, rank=0)
    with pytest.raises(ValueError, match="data parallel"):
        kppo.PPO(_fake_env(), kppo.PPOConfig(target_kl=0.02), dist=dist)
    with pytest.raises(_SetupReached):      # without a target the same call goes on to the device work
        kppo.PPO(_fake_env(), kppo.PPOConfig(), dist=dist)
    with pytest.raises(_SetupReached):
        kppo.PPO(_fake_env(), kppo.PPOConfig(target_kl=0.02))


def test_refused_with_a_teacher_anchor_before_setup(monkeypatch):
    _no_setup(monkeypatch)
    from rl_brain_trainer_amd.teacher_anchor import PopulationTeacherAnchor

    anchor = object.__new__(PopulationTeacherAnchor)
    check = kpop.PopulationPPO._check_population_args
    with pytest.raises(ValueError, match="teacher anchor"):
        check([1, 2], kppo.PPOConfig(target_kl=0.02), None, anchor, None, accepts_anchor=True)
    with pytest.raises(ValueError, match="teacher anchor"):
        check([1, 2], kppo.PPOConfig(), None, anchor, [{"target_kl": 0.02}, {"target_kl": None}], accepts_anchor=True)
    seeds, _, overrides = check([1, 2], kppo.PPOConfig(), None, anchor, None, accepts_anchor=True)
    assert seeds == [1, 2] and overrides == [{}, {}]
    # the single trainer's anchor refuses a gated trainer before it reads its dataset
    from rl_brain_trainer_amd.teacher_anchor import RouteTeacherAnchor, TeacherAnchorConfig

    single = RouteTeacherAnchor(TeacherAnchorConfig(enabled=True, dataset_path="/nonexistent/anchor.npz"))
    with pytest.raises(ValueError, match="target_kl"):
        single.on_training_start(types.SimpleNamespace(kl_targets=[0.02]))


def test_target_kl_is_sweepable():
    assert "target_kl" in kpop.SWEEPABLE
    assert kpop.parse_sweep(["target_kl=0.01,0.03,none"]) == [("target_kl", [0.01, 0.03, None])]
    with pytest.raises(ValueError, match="numbers"):
        kpop.parse_sweep(["learning_rate=1e-4,none"])      # only target_kl takes none
    for key in kpop.SHAPE_KEYS:
        with pytest.raises(ValueError, match="geometry"):
            kpop.parse_sweep([f"{key}=1,2"])
    seeds, overrides, names = kpop.plan_replicas("7", ["target_kl=0.01,none"])
    assert seeds == [7, 7] and overrides == [{"target_kl": 0.01}, {"target_kl": None}]
    assert names == ["seed_7_target_kl_0.01", "seed_7_target_kl_none"]
    assert kpop.check_overrides([1, 2], [{"target_kl": "none"}, {"target_kl": 0.02}]) == [{"target_kl": None}, {"target_kl": 0.02}]
    with pytest.raises(ValueError, match="positive"):
        kpop.check_overrides([1], [{"target_kl": 0.0}])
    with pytest.raises(ValueError, match="distinct"):
        kpop.check_overrides([1, 1], [{"target_kl": None}, {"target_kl": None}])


class _FakeMlp:
    """stands in for mlp.MlpKernels: records what the trainer asks of the handle"""

    def __init__(self, hidden, device, max_batch=8192, obs_dim=56, replicas=1):
        self.hidden, self.replicas, self.train_tile, self.fused, self.kl_gate, self.calls = hidden, replicas, False, True, False, []

    def pack(self, flat):
        self.calls.append("pack")

    def set_train_tile(self, on):
        self.train_tile = bool(on)

    def set_step_count(self, steps):
        self.calls.append(("set_step_count", steps))

    def set_kl_gate(self, targets):
        self.calls.append(("set_kl_gate", list(targets)))
        self.kl_gate = True

    def kl_gate_arm(self):
        self.calls.append("kl_gate_arm")

    def kl_gate_read(self, stream=None):
        self.calls.append("kl_gate_read")
        rec = {"threshold": 0.03, "stopped": 1, "n_counted": 6, "n_seen": 8, "stop_index": 5, "stop_kl": 0.25}
        return [dict(rec) for _ in range(self.replicas)], [5] * self.replicas


class _FakeEvent:
    def record(self, stream=None):
        pass


def _fake_trainer(monkeypatch, target_kl):
    monkeypatch.delenv("KP1_TRAIN_TILE", raising=False)
    monkeypatch.setattr(native, "load", lambda: types.SimpleNamespace())
    monkeypatch.setattr(kmlp, "MlpKernels", _FakeMlp)
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: types.SimpleNamespace(wait_event=lambda ev: None))
    monkeypatch.setattr(torch.cuda, "Event", _FakeEvent)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    env = types.SimpleNamespace(device=torch.device("cpu"), n_envs=4, obs_dim=56, set_obs_stride=lambda w: None)
    p = object.__new__(kppo.PPO)
    cfg = kppo.PPOConfig(n_steps=4, batch_size=4, n_epochs=2, hidden=64, target_kl=target_kl)
    p._setup(cfg, [0], [env], [None], kppo.Dist(), False, min_batch=64, stacked=False)
    p.policy = p.policies[0]
    p._setup_kl_gate(kppo.check_target_kl([cfg.target_kl], p.dist))
    epochs = []
    p._epoch_body = lambda: epochs.append(1)
    p._draw_perm = lambda k: None
    return p, epochs


def test_a_trainer_without_a_target_makes_no_gate_call(monkeypatch):
    p, epochs = _fake_trainer(monkeypatch, None)
    p.train()
    p.train()
    assert p.kl_targets is None and len(epochs) == 4
    assert not [c for c in p._mlp.calls if "kl_gate" in str(c)]
    assert p._mlp.calls.count(("set_step_count", 0)) == 1 and p.adam_t == 4 * 4      # the eager epochs push the host mirror, as before
    assert p.n_updates() == 4 and p.adam_step_count() == 16
    assert not any(isinstance(e, tuple) and e and e[0] == "kl_gate" for e in p._epoch_key())
    with pytest.raises(RuntimeError, match="target_kl"):
        p.kl_stops()


def test_a_gated_trainer_arms_once_per_train_and_resolves_lazily(monkeypatch):
    p, epochs = _fake_trainer(monkeypatch, 0.02)
    assert p._mlp.calls == ["pack", ("set_kl_gate", [0.02])]
    p.train()
    assert p._mlp.calls.count("kl_gate_arm") == 1 and len(epochs) == 2 and "kl_gate_read" not in p._mlp.calls
    assert not [c for c in p._mlp.calls if isinstance(c, tuple) and c[0] == "set_step_count"]      # the device's counts are the truth
    stops = p.kl_stops()
    assert stops == [{"early_stop": True, "stop_epoch": 1, "stop_minibatch": 1, "stop_kl": 0.25}]
    assert p._mlp.calls.count("kl_gate_read") == 1 and p.adam_step_count() == 5 and p.adam_t == 5 and p.n_updates() == 2
    p.kl_stops()
    assert p._mlp.calls.count("kl_gate_read") == 1          # resolved once per train() call
    p.train()
    assert p._mlp.calls.count("kl_gate_arm") == 2
    assert p.n_updates() == 4 and p._mlp.calls.count("kl_gate_read") == 2


def test_epoch_key_keeps_the_train_tile_flag_last(monkeypatch):
    for target in (None, 0.02):
        p, _ = _fake_trainer(monkeypatch, target)
        assert p._epoch_key()[-1] is False
        p._mlp.set_train_tile(True)
        assert p._epoch_key()[-1] is True
    gated, _ = _fake_trainer(monkeypatch, 0.02)
    plain, _ = _fake_trainer(monkeypatch, None)
    assert ("kl_gate", (0.02,)) in gated._epoch_key() and len(gated._epoch_key()) == len(plain._epoch_key()) + 1


def test_logger_prints_the_early_stopping_line():
    out = io.StringIO()
    log = kmon.TrainLogger(out=out)
    row = log.log({"train/n_updates": 6, "train/approx_kl": 0.04, "kl_stop": {"stop_epoch": 1, "stop_minibatch": 2, "stop_kl": 0.0449}},
                  iteration=3, total_timesteps=3072)
    text = out.getvalue()
    assert text.startswith("Early stopping at step 1 due to reaching max kl: 0.04\n")
    assert row["train/n_updates"] == 6 and "kl_stop" not in row and re.search(r"n_updates\s*\|\s*6\b", text)
    out = io.StringIO()
    kmon.TrainLogger(out=out).log({"train/n_updates": 8}, iteration=4, total_timesteps=4096)
    assert "Early stopping" not in out.getvalue()
