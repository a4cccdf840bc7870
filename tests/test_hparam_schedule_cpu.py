"""Learning-rate and clip-range schedules, the host side without a device: the C symbol and its binding against the
header's text, SB3's LinearSchedule restated, the config fields and every refusal before device work, the progress clock of the training
loop (on fakes), what a scheduled trainer asks of its MLP handle, the epoch graph key, the pickle stream of the schedule payload and the
logger's row."""
from __future__ import annotations

import base64
import dataclasses
import inspect
import io
import math
import pickle
import pickletools
import re
import sys
import types

import pytest
import torch
import yaml

import abi
from rl_brain_trainer_amd import checkpoint
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import mlp as kmlp
from rl_brain_trainer_amd import monitor as kmon
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import population as kpop
from rl_brain_trainer_amd import ppo as kppo
from rl_brain_trainer_amd import sb3_pickle as sbp


def _header() -> str:
    return abi.header("kp1_ppo.h")


def test_symbol_declared_exported_and_bound():
    args = abi.params("kp1_mlp_hparams_store", "kp1_ppo.h")      # raises if include/kp1_ppo.h does not declare it
    assert args == ["kp1_mlp* m", "const kp1_replica_hparams* host", "int32_t n", "void* stream"]
    assert "kp1_mlp_hparams_store" in native.declared_symbols()
    L = native.load()
    assert hasattr(L, "kp1_mlp_hparams_store"), "libkp1.so does not export kp1_mlp_hparams_store"
    import ctypes as C

    assert list(L.kp1_mlp_hparams_store.argtypes) == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    # the table's entry is six floats in the order the Python side writes them
    s = re.search(r"typedef\s+struct\s+kp1_replica_hparams\s*\{(.*?)\}", _header(), flags=re.S).group(1)
    assert [n.strip() for n in s.replace("float", "").strip(" ;\n").split(",")] == list(kmlp.MlpKernels.HPARAM_FIELDS)


def _sb3_linear(start, end, end_fraction, p):
    """stable_baselines3.common.utils.LinearSchedule.__call__, restated"""
    if (1 - p) > end_fraction:
        return end
    return start + (1 - p) * (end - start) / end_fraction


def test_linear_schedule_formula():
    f = kppo.linear_schedule
    assert f(3e-4, 0.0, 1.0, 1.0) == 3e-4                      # p = 1: the start
    assert f(3e-4, 0.0, 1.0, 0.0) == 0.0                       # p = 0 with the whole run as the ramp: the end
    assert f(0.2, 0.05, 0.5, 0.0) == 0.05                      # p = 0 behind the ramp
    # exactly at 1 - p == end_fraction the interpolated branch is taken (the comparison is strict) and lands on the end
    assert (1 - 0.5) == 0.5 and f(0.2, 0.05, 0.5, 0.5) == 0.2 + 0.5 * (0.05 - 0.2) / 0.5
    # (three rounded operations on magnitudes of at most 0.2: within 3 * 0.5 ulp(0.2) of the end, not necessarily on it)
    assert abs(f(0.2, 0.05, 0.5, 0.5) - 0.05) <= 1.5 * math.ulp(0.2)
    # just beyond: the end itself, not an extrapolation
    p = 0.5 - math.ulp(0.5)          # 1 - p is the double just above 0.5 (one ulp of 0.5 is the spacing above it)
    assert (1 - p) > 0.5 and f(0.2, 0.05, 0.5, p) == 0.05
    for start, end, frac in ((3e-4, 0.0, 1.0), (0.2, 0.05, 0.5), (1e-4, 3e-6, 0.25)):
        for k in range(0, 33):
            p = 1.0 - k / 32.0
            assert f(start, end, frac, p) == _sb3_linear(start, end, frac, p)
            assert isinstance(f(start, end, frac, p), float)


def test_config_fields_and_order():
    cfg = kppo.PPOConfig()
    assert cfg.learning_rate_schedule is None and cfg.clip_range_schedule is None
    params = list(inspect.signature(kppo.PPOConfig).parameters.values())
    names = [p.name for p in params]
    # behind target_kl in the constructor, and keyword-only: positional use of every older field is unchanged
    assert names[-3:] == ["target_kl", "learning_rate_schedule", "clip_range_schedule"]
    assert [p.kind for p in params[-2:]] == [inspect.Parameter.KEYWORD_ONLY] * 2
    assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params[:-2])
    assert names[:16] == ["learning_rate", "n_steps", "batch_size", "n_epochs", "gamma", "gae_lambda", "clip_range", "ent_coef", "vf_coef",
                          "max_grad_norm", "adam_eps", "seed", "hidden", "normalize_advantage", "total_timesteps", "target_kl"]
    assert kppo.PPOConfig(1e-4, 64).n_steps == 64
    assert "learning_rate_schedule" not in kpop.SWEEPABLE and "clip_range_schedule" not in kpop.SWEEPABLE
    repl = dataclasses.replace(kppo.PPOConfig(learning_rate_schedule={"end": 0.0, "end_fraction": 1.0}), seed=3, learning_rate=1e-4)
    assert repl.learning_rate_schedule == {"end": 0.0, "end_fraction": 1.0} and repl.learning_rate == 1e-4


def test_config_from_a_yaml_block():
    block = yaml.safe_load("""
algorithms:
  ppo:
    learning_rate: 1.0e-4
    clip_range: 0.2
    learning_rate_schedule: {end: 0.0, end_fraction: 1.0}
    clip_range_schedule: {end: 0.05, end_fraction: 0.5}
""")["algorithms"]["ppo"]
    cfg = kppo.PPOConfig.from_algo_kwargs(block, hidden=64)
    assert cfg.learning_rate == 1e-4 and cfg.learning_rate_schedule == {"end": 0.0, "end_fraction": 1.0}
    assert kppo.check_schedules(cfg) == {"learning_rate": {"end": 0.0, "end_fraction": 1.0}, "clip_range": {"end": 0.05, "end_fraction": 0.5}}
    assert kppo.check_schedules(kppo.PPOConfig()) is None
    assert kppo.check_schedules(kppo.PPOConfig(clip_range_schedule={"end": 0.1, "end_fraction": 1})) == {"clip_range": {"end": 0.1, "end_fraction": 1.0}}


class _SetupReached(Exception):
    pass


def _fake_env():
    return types.SimpleNamespace(dtype=torch.float32, is_population=False, device=torch.device("cpu"), n_envs=4)


BAD = [
    ("learning_rate_schedule", {"end": 0.0, "end_fraction": 1.0, "start": 1e-3}, "unknown keys"),
    ("learning_rate_schedule", {"end": 0.0}, "missing"),
    ("learning_rate_schedule", {"end": float("nan"), "end_fraction": 1.0}, "finite"),
    ("learning_rate_schedule", {"end": 0.0, "end_fraction": float("inf")}, "finite"),
    ("learning_rate_schedule", {"end": 0.0, "end_fraction": 0.0}, "end_fraction"),
    ("learning_rate_schedule", {"end": 0.0, "end_fraction": 1.5}, "end_fraction"),
    ("learning_rate_schedule", {"end": 0.0, "end_fraction": -0.5}, "end_fraction"),
    ("learning_rate_schedule", {"end": -1e-6, "end_fraction": 1.0}, ">= 0"),
    ("learning_rate_schedule", "lin_3e-4", "mapping"),
    ("clip_range_schedule", {"end": 0.0, "end_fraction": 1.0}, "> 0"),
    ("clip_range_schedule", {"end": -0.1, "end_fraction": 1.0}, "> 0"),
    ("clip_range_schedule", {"end": 0.1, "end_fraction": 1.0, "lin": 1}, "unknown keys"),
    ("clip_range_schedule", {"end": float("inf"), "end_fraction": 1.0}, "finite"),
]


@pytest.mark.parametrize("fld,value,words", BAD)
def test_refusals_before_setup(monkeypatch, fld, value, words):
    def boom(self, *a, **k):
        raise _SetupReached()

    monkeypatch.setattr(kppo.PPO, "_setup", boom)
    with pytest.raises(ValueError, match=words):
        kppo.PPO(_fake_env(), kppo.PPOConfig(**{fld: value}))
    with pytest.raises(ValueError, match=words):
        kpop.PopulationPPO._check_population_args([1, 2], kppo.PPOConfig(**{fld: value}), None, None, None)


def test_accepted_schedules_reach_setup_also_under_data_parallel(monkeypatch):
    def boom(self, *a, **k):
        raise _SetupReached()

    monkeypatch.setattr(kppo.PPO, "_setup", boom)
    cfg = kppo.PPOConfig(learning_rate_schedule={"end": 0.0, "end_fraction": 1.0}, clip_range_schedule={"end": 0.05, "end_fraction": 0.5})
    with pytest.raises(_SetupReached):
        kppo.PPO(_fake_env(), cfg)
    with pytest.raises(_SetupReached):      # data parallel is allowed: every rank evaluates the same value on the global clock
        kppo.PPO(_fake_env(), cfg, dist=types.SimpleNamespace(enabled=True, world_size=2, rank=0))


def test_refused_with_a_teacher_anchor():
    from rl_brain_trainer_amd.teacher_anchor import PopulationTeacherAnchor, RouteTeacherAnchor, TeacherAnchorConfig

    anchor = object.__new__(PopulationTeacherAnchor)
    check = kpop.PopulationPPO._check_population_args
    cfg = kppo.PPOConfig(learning_rate_schedule={"end": 0.0, "end_fraction": 1.0})
    with pytest.raises(ValueError, match="teacher anchor"):
        check([1, 2], cfg, None, anchor, None, accepts_anchor=True)
    check([1, 2], cfg, None, None, None)
    check([1, 2], kppo.PPOConfig(), None, anchor, None, accepts_anchor=True)
    single = RouteTeacherAnchor(TeacherAnchorConfig(enabled=True, dataset_path="/nonexistent/anchor.npz"))
    with pytest.raises(ValueError, match="schedule"):
        single.on_training_start(types.SimpleNamespace(kl_targets=None, hparam_schedules={"learning_rate": {"end": 0.0, "end_fraction": 1.0}}))


# ---------------------------------------------------------------------------------------------- the training loop's clock, on fakes
class _FakeLoopTrainer:
    monitor = None

    def __init__(self, clock: int, per_rollout: int, world: int = 1):
        self.num_timesteps, self.per_rollout, self.events = clock, per_rollout, []
        self.progress_remaining = 1.0
        self.dist = types.SimpleNamespace(rank=0, world_size=world, enabled=world > 1)
        self.device = None

    def collect_rollouts(self):
        self.events.append(("collect", self.progress_remaining))
        self.num_timesteps += self.per_rollout * self.dist.world_size       # the clock counts all ranks

    def train(self):
        self.events.append(("train", self.progress_remaining, self.num_timesteps))


def test_run_training_sets_progress_between_rollout_and_train(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)
    t = _FakeLoopTrainer(0, 1024)
    seen = []
    kppo.run_training(t, 3072, after_rollout=lambda tr: seen.append(tr.progress_remaining))
    trains = [e for e in t.events if e[0] == "train"]
    assert [e[1] for e in trains] == [1.0 - 1024.0 / 3072.0, 1.0 - 2048.0 / 3072.0, 1.0 - 3072.0 / 3072.0]
    # collect_rollouts and after_rollout of an iteration still see the previous value: it is set behind both
    assert [e[1] for e in t.events if e[0] == "collect"] == [1.0, trains[0][1], trains[1][1]] and seen == [1.0, trains[0][1], trains[1][1]]
    # resume (reset_num_timesteps=False): the total is the clock as the loop found it plus the requested steps
    t = _FakeLoopTrainer(5000, 512)
    kppo.run_training(t, 1024)
    assert [e[1] for e in t.events if e[0] == "train"] == [1.0 - 5512.0 / 6024.0, 1.0 - 6024.0 / 6024.0]
    # data parallel: the global clock
    t = _FakeLoopTrainer(0, 512, world=2)
    kppo.run_training(t, 2048)
    assert [e[1] for e in t.events if e[0] == "train"] == [0.5, 0.0]


# ---------------------------------------------------------------------------------------------- what a trainer asks of its handle
class _FakeMlp:
    HPARAM_FIELDS = kmlp.MlpKernels.HPARAM_FIELDS

    def __init__(self, hidden, device, max_batch=8192, obs_dim=56, replicas=1):
        self.hidden, self.replicas, self.train_tile, self.fused, self.kl_gate, self.calls = hidden, replicas, False, True, False, []

    def pack(self, flat):
        self.calls.append("pack")

    def set_train_tile(self, on):
        self.train_tile = bool(on)

    def set_step_count(self, steps):
        self.calls.append(("set_step_count", steps))

    def hparams_store(self, rows):
        self.calls.append(("hparams_store", [dict(r) for r in rows]))


def _fake_trainer(monkeypatch, world: int = 1, **cfg_kw):
    monkeypatch.delenv("KP1_TRAIN_TILE", raising=False)
    monkeypatch.setattr(native, "load", lambda: types.SimpleNamespace())
    monkeypatch.setattr(kmlp, "MlpKernels", _FakeMlp)
    env = types.SimpleNamespace(device=torch.device("cpu"), n_envs=4, obs_dim=56, set_obs_stride=lambda w: None)
    p = object.__new__(kppo.PPO)
    cfg = kppo.PPOConfig(n_steps=4, batch_size=4, n_epochs=2, hidden=64, learning_rate=1e-3, clip_range=0.2, ent_coef=0.01, **cfg_kw)
    dist = kppo.Dist()
    if world > 1:
        dist = types.SimpleNamespace(enabled=True, world_size=world, rank=0, broadcast=lambda t: None, use_stream_collectives=lambda d: None,
                                     graph_mode=lambda d: "none")
    p._setup(cfg, [0], [env], [None], dist, False, min_batch=64, stacked=False)
    p.policy = p.policies[0]
    p._setup_kl_gate(kppo.check_target_kl([cfg.target_kl], kppo.Dist()))
    p._setup_schedules(kppo.check_schedules(cfg))
    epochs = []
    p._epoch_body = lambda: epochs.append(1)
    p._draw_perm = lambda k: None
    return p, epochs


SCHED = dict(learning_rate_schedule={"end": 0.0, "end_fraction": 1.0}, clip_range_schedule={"end": 0.05, "end_fraction": 0.5})


def test_one_store_per_train_with_the_values_of_the_formula(monkeypatch):
    p, epochs = _fake_trainer(monkeypatch, **SCHED)
    assert p.hparam_schedules == {"learning_rate": SCHED["learning_rate_schedule"], "clip_range": SCHED["clip_range_schedule"]}
    assert p.current_hparams() == {"learning_rate": 1e-3, "clip_range": 0.2}        # before the first train(): the starts
    stores = lambda: [c[1] for c in p._mlp.calls if isinstance(c, tuple) and c[0] == "hparams_store"]     # noqa: E731
    for n, prog in enumerate((0.75, 0.5, 0.25), start=1):
        p.progress_remaining = prog
        p.train()
        assert len(stores()) == n and len(epochs) == 2 * n
        (row,) = stores()[-1]
        assert row == {"learning_rate": _sb3_linear(1e-3, 0.0, 1.0, prog), "clip_range": _sb3_linear(0.2, 0.05, 0.5, prog), "adam_eps": 1e-5,
                       "max_grad_norm": 0.5, "ent_coef": 0.01, "vf_coef": 0.5}
        assert p.current_hparams() == {"learning_rate": row["learning_rate"], "clip_range": row["clip_range"]}
    assert stores()[-1][0]["clip_range"] == 0.05      # behind the ramp


def test_one_schedule_leaves_the_other_constant_and_data_parallel_divides_ent_coef(monkeypatch):
    p, _ = _fake_trainer(monkeypatch, world=2, learning_rate_schedule={"end": 1e-4, "end_fraction": 1.0})
    p.progress_remaining = 0.5
    p.train()
    (row,) = [c[1] for c in p._mlp.calls if isinstance(c, tuple) and c[0] == "hparams_store"][-1]
    assert row["learning_rate"] == _sb3_linear(1e-3, 1e-4, 1.0, 0.5) and row["clip_range"] == 0.2 and row["ent_coef"] == 0.01 / 2


def test_no_schedule_no_store_and_the_parents_key(monkeypatch):
    plain, _ = _fake_trainer(monkeypatch)
    none, _ = _fake_trainer(monkeypatch, learning_rate_schedule=None, clip_range_schedule=None)
    for p in (plain, none):
        p.progress_remaining = 0.5
        p.train()
        assert p.hparam_schedules is None and not [c for c in p._mlp.calls if isinstance(c, tuple) and c[0] == "hparams_store"]
        assert p.current_hparams() == {"learning_rate": 1e-3, "clip_range": 0.2}
    c = plain.cfg
    assert plain._epoch_key() == none._epoch_key() == (c.learning_rate, c.clip_range, c.ent_coef, c.vf_coef, c.max_grad_norm, c.adam_eps, c.batch_size,
                                                       c.n_steps, c.normalize_advantage, 1, False)


def test_epoch_key_of_a_scheduled_trainer_is_free_of_the_values(monkeypatch):
    p, _ = _fake_trainer(monkeypatch, **SCHED)
    key = p._epoch_key()
    assert ("hparam_line", ("clip_range", "learning_rate")) in key and key[-1] is False
    p.progress_remaining = 0.25
    p.train()
    assert p._epoch_key() == key
    p.cfg.learning_rate, p.cfg.clip_range = 5e-4, 0.1          # the starts: read from the table too, so not part of what a capture froze
    assert p._epoch_key() == key
    assert not any(isinstance(e, float) and e in (1e-3, 0.2, 5e-4, 0.1) for e in key)
    p._mlp.set_train_tile(True)
    assert p._epoch_key()[-1] is True
    gated, _ = _fake_trainer(monkeypatch, target_kl=None, **SCHED)
    gated.kl_targets = [0.02]
    k2 = gated._epoch_key()
    assert k2[-2] == ("kl_gate", (0.02,)) and k2[-3][0] == "hparam_line" and k2[-1] is False


# ---------------------------------------------------------------------------------------------- the checkpoint's schedule payload
def test_linear_schedule_payload_opcodes_and_rebuild(monkeypatch):
    payload = sbp.serialized(sbp.linear_schedule(3e-4, 0.0, 0.75))
    assert sbp.describe(payload) == [("stable_baselines3.common.utils", "FloatSchedule"), ("stable_baselines3.common.utils", "LinearSchedule")]
    raw = base64.b64decode(payload)
    ops = [(op.name, arg) for op, arg, _ in pickletools.genops(raw)]
    assert ops[0] == ("PROTO", 2) and ops[-1][0] == "STOP"
    assert b"rl_brain_trainer_amd" not in raw
    strings = [arg for name, arg in ops if name in ("BINUNICODE", "SHORT_BINUNICODE", "UNICODE")]
    assert set(strings) == {"value_schedule", "start", "end", "end_fraction"}
    assert sorted(arg for name, arg in ops if name == "BINFLOAT") == [0.0, 3e-4, 0.75]
    # rebuilt under empty modules of the real names (nothing of SB3 is imported or unpickled): plain classes whose __dict__ gets the state
    utils = types.ModuleType("stable_baselines3.common.utils")
    utils.FloatSchedule = type("FloatSchedule", (), {"__module__": utils.__name__})
    utils.LinearSchedule = type("LinearSchedule", (), {"__module__": utils.__name__})
    for name, mod in (("stable_baselines3", types.ModuleType("stable_baselines3")), ("stable_baselines3.common", types.ModuleType("stable_baselines3.common")),
                      (utils.__name__, utils)):
        monkeypatch.setitem(sys.modules, name, mod)
    obj = pickle.loads(raw)
    assert type(obj) is utils.FloatSchedule and type(obj.value_schedule) is utils.LinearSchedule
    assert obj.value_schedule.__dict__ == {"start": 3e-4, "end": 0.0, "end_fraction": 0.75}
    # the constant payload is what it was
    assert sbp.describe(sbp.serialized(sbp.float_schedule(3e-4)))[1] == ("stable_baselines3.common.utils", "ConstantSchedule")


def test_checkpoint_entries():
    e = checkpoint._schedule_entry(3e-4, {"end": 0.0, "end_fraction": 1.0})
    assert e["value"] == 3e-4 and e["end"] == 0.0 and e["end_fraction"] == 1.0 and e[":type:"].endswith("FloatSchedule'>")
    assert e[":serialized:"] == sbp.serialized(sbp.linear_schedule(3e-4, 0.0, 1.0))
    c = checkpoint._schedule_entry(3e-4, None)
    assert c == {":type:": "<class 'stable_baselines3.common.utils.FloatSchedule'>", ":serialized:": sbp.serialized(sbp.float_schedule(3e-4)), "value": 3e-4}
    assert list(c) == [":type:", ":serialized:", "value"]          # key order is part of the archive's bytes


def test_monitor_row_and_logger_show_the_values_the_last_train_used(monkeypatch):
    """monitor_rows() of a scheduled trainer (fake handle, fake monitor: no episode has ended) reports current_hparams(k), and the
    logger prints that row's values"""
    p, _ = _fake_trainer(monkeypatch, **SCHED)
    p.monitor = types.SimpleNamespace(read=lambda k: native.MonitorState())
    p._ev_dev = torch.zeros((1, 2), dtype=torch.float64)
    p._log_std_snap = torch.zeros((1, 7), dtype=torch.float32)
    p._stats_rows = lambda: [{}]
    (row,) = p.monitor_rows()
    assert (row["train/learning_rate"], row["train/clip_range"]) == (1e-3, 0.2)          # before the first train(): the starts
    p.progress_remaining = 0.25
    p.train()
    lr, clip = _sb3_linear(1e-3, 0.0, 1.0, 0.25), _sb3_linear(0.2, 0.05, 0.5, 0.25)
    assert (lr, clip) == (0.00025, 0.05) and p.cfg.learning_rate == 1e-3 and p.cfg.clip_range == 0.2
    (row,) = p.monitor_rows()
    assert (row["train/learning_rate"], row["train/clip_range"], row["train/n_updates"]) == (lr, clip, 2)
    out = io.StringIO()
    logged = kmon.TrainLogger(out=out).log(row, iteration=1, total_timesteps=16)
    assert logged["train/learning_rate"] == lr and logged["train/clip_range"] == clip
    text = out.getvalue()
    assert re.search(r"learning_rate\s*\|\s*0\.00025\b", text) and re.search(r"clip_range\s*\|\s*0\.05\b", text)


def test_set_replica_hparams_still_refuses_k1_in_the_source():
    """the K = 1 refusal of the older entry point stays (tests/test_population_sweep_gpu.py pins it on the device); here: its text is still
    in the entry point, in front of the copy, and the new entry point has no such refusal"""
    src = (kcfg.repo_root() / "rl_brain_trainer_amd" / "csrc" / "kp1_mlp.hip").read_text()
    old = src[src.index("int kp1_mlp_set_replica_hparams("):]
    old = old[:old.index("\n}\n")]
    assert 'if (m->K == 1) return fail(KP1_ERR_UNSUPPORTED, "a K = 1 handle takes its hyper-parameters as scalar arguments' in old
    assert old.index("m->K == 1") < old.index("hipMemcpyAsync")
    new = src[src.index('int kp1_mlp_hparams_store('):]
    new = new[:new.index("\n}\n")]
    assert "n != m->K" in new and "hipMemcpy" not in new and "Synchronize" not in new and "isfinite" in new
