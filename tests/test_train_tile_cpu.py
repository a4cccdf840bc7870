"""Host side of the one-launch training tile (KP1_MLP_OPT_TRAIN_TILE) without a GPU: the coverage predicate on plain
values, the switch and its default, the chunk function, PPO's call of ``set_train_tile`` on a fake library, and the three CLI flags."""
from __future__ import annotations

import types

import pytest
import torch

from rl_brain_trainer_amd import mlp as kmlp
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import population as kpop
from rl_brain_trainer_amd import ppo as kppo


def test_predicate_on_plain_values():
    assert kppo.train_tile_covered(64, "1") and kppo.train_tile_covered(128, "1")
    assert not kppo.train_tile_covered(256, "1")            # its own tile path
    assert not kppo.train_tile_covered(32, "1")
    assert kppo.TRAIN_TILE_WIDTHS == (64, 128) and kppo.TRAIN_TILE_ENV == "KP1_TRAIN_TILE"


def test_switch_and_default():
    for hidden in (64, 128):
        assert not kppo.train_tile_covered(hidden, None)    # unset: the trainer's default, which is off
        assert not kppo.train_tile_covered(hidden, "0")
        assert kppo.train_tile_covered(hidden, "1")
        assert not kppo.train_tile_covered(hidden, "yes")   # "1" and nothing else
        assert kppo.train_tile_covered(hidden, None, default_on=True)
        assert not kppo.train_tile_covered(hidden, "0", default_on=True)
    assert not kppo.train_tile_covered(256, None, default_on=True)
    # no trainer has the tile as its default (not decided by a measurement yet)
    for cls in (kppo.PPO, kpop.PopulationPPO, kpop.ApproachPopulationPPO, kpop.RoutePopulationPPO, kpop.DockPopulationPPO):
        assert cls.train_tile_default is False


def test_chunk_function():
    """n -> chunks of one 32-row tile, or 0 = the layer-wise launches; a function of n alone"""
    assert [kppo.train_tile_chunks(n) for n in (1, 32, 33, 2048, 2049)] == [1, 1, 2, 64, 0]
    assert kppo.train_tile_chunks(0) == 0 and kppo.train_tile_chunks(256) == 8 and kppo.train_tile_chunks(520) == 17
    assert kppo.TRAIN_TILE_MAX_ROWS == 2048 and all(kppo.train_tile_chunks(n) <= 64 for n in range(1, 4100))


class _FakeMlp:
    """stands in for mlp.MlpKernels in PPO._setup: records the option calls"""
    made: list["_FakeMlp"] = []

    def __init__(self, hidden, device, max_batch=8192, obs_dim=56, replicas=1):
        self.hidden, self.replicas, self.train_tile, self.fused, self.calls = hidden, replicas, False, True, []
        _FakeMlp.made.append(self)

    def pack(self, flat):
        self.calls.append("pack")

    def set_train_tile(self, on):
        self.calls.append(("set_train_tile", on))
        self.train_tile = bool(on)


def _setup_ppo(monkeypatch, hidden: int, K: int = 1):
    monkeypatch.setattr(native, "load", lambda: types.SimpleNamespace())
    monkeypatch.setattr(kmlp, "MlpKernels", _FakeMlp)
    _FakeMlp.made.clear()
    envs = [types.SimpleNamespace(device=torch.device("cpu"), n_envs=4, obs_dim=56, set_obs_stride=lambda w: None) for _ in range(K)]
    p = object.__new__(kppo.PPO)
    p._setup(kppo.PPOConfig(n_steps=4, batch_size=8, hidden=hidden), list(range(K)), envs, [None] * K, kppo.Dist(), False, min_batch=64, stacked=K > 1)
    assert len(_FakeMlp.made) == 1 and p._mlp is _FakeMlp.made[0] and p._mlp.replicas == K
    return p


@pytest.mark.parametrize("K", (1, 3))
def test_ppo_sets_the_option(monkeypatch, K):
    """PPO._setup serves K = 1 and every population class: one site"""
    monkeypatch.setenv("KP1_TRAIN_TILE", "1")
    for hidden in (64, 128):
        p = _setup_ppo(monkeypatch, hidden, K)
        assert p._mlp.calls == ["pack", ("set_train_tile", True)]
        assert p.update_form.startswith("train tile") and p._epoch_key()[-1] is True
    p = _setup_ppo(monkeypatch, 256, 1)
    assert p._mlp.calls == ["pack"] and p.update_form.startswith("tile 2x256")
    for var in (None, "0"):
        if var is None:
            monkeypatch.delenv("KP1_TRAIN_TILE")
        else:
            monkeypatch.setenv("KP1_TRAIN_TILE", var)
        p = _setup_ppo(monkeypatch, 64, K)
        assert p._mlp.calls == ["pack"] and p.update_form == "layer-wise" and p._epoch_key()[-1] is False


def test_epoch_graph_key_follows_a_toggle(monkeypatch):
    monkeypatch.delenv("KP1_TRAIN_TILE", raising=False)
    p = _setup_ppo(monkeypatch, 64)
    before = p._epoch_key()
    p._mlp.set_train_tile(True)
    assert p._epoch_key() != before


def test_mlp_kernels_sets_option_6():
    calls = []
    m = object.__new__(kmlp.MlpKernels)
    m.L = types.SimpleNamespace(kp1_mlp_set_option=lambda h, opt, val: calls.append((opt, val)) or 0)
    m._h, m.train_tile = None, False
    m.set_train_tile(True)
    assert calls == [(6, 1)] and m.train_tile is True and kmlp.MlpKernels.OPT_TRAIN_TILE == 6
    m.set_train_tile(False)
    assert calls[-1] == (6, 0) and m.train_tile is False


def test_cli_flags():
    from rl_brain_trainer_amd import train, train_dock, train_route

    for mod in (train, train_dock, train_route):
        parser = mod.build_arg_parser()
        flag = next(a for a in parser._actions if "--train-tile" in a.option_strings)
        assert flag.dest == "train_tile" and flag.default is False and flag.const is True
