"""The host side of the one-launch rollout step without a GPU: the predicate that chooses it (ppo.fused_rollout_covered) on plain values, and
which path the one-handle populations take, on fakes."""
from __future__ import annotations

import pytest
import torch

from rl_brain_trainer_amd import population as pop_mod
from rl_brain_trainer_amd import ppo as ppo_mod
from rl_brain_trainer_amd.ppo import PPOConfig, fused_rollout_covered

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("hidden", [64, 128, 256])
def test_predicate_covers_the_three_widths(hidden):
    assert fused_rollout_covered(True, F32, hidden, 56, False, "1")
    assert not fused_rollout_covered(True, F32, hidden, 56, False, "0")            # KP1_FUSED_ROLLOUT=0 keeps the launch sequence
    assert not fused_rollout_covered(False, F32, hidden, 56, False, "1")           # an env the entry point does not step
    assert not fused_rollout_covered(True, F64, hidden, 56, False, "1")            # the f64 env
    assert not fused_rollout_covered(True, F32, hidden, 80, False, "1")            # the route observation
    assert not fused_rollout_covered(True, F32, hidden, 56, True, "1")             # recorded reward components
    # unset: the calling trainer's default
    assert fused_rollout_covered(True, F32, hidden, 56, False, None, default_on=True)
    assert not fused_rollout_covered(True, F32, hidden, 56, False, None, default_on=False)
    assert not fused_rollout_covered(True, F32, hidden, 56, True, None, default_on=True)
    assert not fused_rollout_covered(True, F32, hidden, 56, False, "0", default_on=True)      # the variable beats the default
    assert fused_rollout_covered(True, F32, hidden, 56, False, "1", default_on=False)


def test_predicate_refuses_other_widths_and_keeps_the_tile_default():
    for hidden in (32, 96, 512):
        assert not fused_rollout_covered(True, F32, hidden, 56, False, "1")
    assert fused_rollout_covered(True, F32, 64, 64, False, "1")                    # (the padded width counts as the 56-float observation)
    assert ppo_mod.FUSED_ROLLOUT_WIDTHS == (64, 128, 256)


class _Cfg:
    def __init__(self, hidden):
        self.hidden = hidden


@pytest.mark.parametrize("hidden,unset", [(256, True), (64, False), (128, False)])
def test_single_seed_ppo_default(hidden, unset, monkeypatch):
    """PPO on an unset KP1_FUSED_ROLLOUT: the 2x256 tile form is the default, the layer-wise widths opt in"""
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    env = object.__new__(ArmKinematicVecEnv)
    env.dtype = F32
    p = object.__new__(ppo_mod.PPO)
    p.env, p.cfg, p.obs_dim = env, _Cfg(hidden), 56
    monkeypatch.delenv("KP1_FUSED_ROLLOUT", raising=False)
    assert p._fused_env_step == unset
    monkeypatch.setenv("KP1_FUSED_ROLLOUT", "1")
    assert p._fused_env_step
    env._reward_components_on = True
    assert not p._fused_env_step
    env._handle = None      # (nothing to close)


class _FakeEnv:
    dtype = F32

    def __init__(self, components: bool = False) -> None:
        self._reward_components_on = components
        self.calls = 0

    def step_into(self, *args) -> None:
        self.calls += 1


class _FakeMlp:
    def __init__(self) -> None:
        self.fused, self.plain = 0, 0

    def forward_env_step(self, env, obs, **kw) -> None:
        assert set(kw) == {"noise", "value", "action", "log_prob", "next_obs", "reward", "done", "terminal_obs"}
        self.fused += 1

    def forward(self, obs, **kw) -> None:
        self.plain += 1


def _fake(cls, *, obs_dim: int = 56, components: bool = False, hidden: int = 64):
    p = object.__new__(cls)
    p.cfg = PPOConfig(n_steps=2, hidden=hidden)
    p.obs_dim = obs_dim
    p.pop_env = _FakeEnv(components)
    p._mlp = _FakeMlp()
    for name in ("obs_buf", "noise_all", "val_buf", "act_buf", "logp_buf", "rew_buf", "done_buf", "term_obs_buf"):
        setattr(p, name, torch.zeros((3, 4, 1)))
    p.clip_act = torch.zeros((4, 7))
    return p


@pytest.mark.parametrize("cls_name,covered", [("ApproachPopulationPPO", True), ("DockPopulationPPO", True), ("RoutePopulationPPO", False),
                                              ("OneHandlePopulationPPO", False)])
def test_one_handle_populations_choose_the_path(cls_name, covered, monkeypatch):
    cls = getattr(pop_mod, cls_name)
    for env_var, want in (("1", covered), ("0", False)):
        monkeypatch.setenv("KP1_FUSED_ROLLOUT", env_var)
        p = _fake(cls, obs_dim=80 if cls_name == "RoutePopulationPPO" else 56)
        p._policy_env_step(0)
        assert (p._mlp.fused, p._mlp.plain, p.pop_env.calls) == ((1, 0, 0) if want else (0, 1, 1)), (cls_name, env_var)
    monkeypatch.delenv("KP1_FUSED_ROLLOUT")           # unset: the Approach and dock populations' measured default is on
    p = _fake(cls, obs_dim=80 if cls_name == "RoutePopulationPPO" else 56)
    p._policy_env_step(0)
    assert (p._mlp.fused, p._mlp.plain, p.pop_env.calls) == ((1, 0, 0) if covered else (0, 1, 1)), cls_name
    monkeypatch.setenv("KP1_FUSED_ROLLOUT", "1")
    p = _fake(cls, components=True)                   # recorded reward components: the env's own step kernel
    p._policy_env_step(0)
    assert (p._mlp.fused, p._mlp.plain, p.pop_env.calls) == (0, 1, 1)


def test_k_handle_population_keeps_the_launch_sequence(monkeypatch):
    """PopulationPPO (one env handle per replica) steps each handle after one forward of all replicas"""
    monkeypatch.setenv("KP1_FUSED_ROLLOUT", "1")
    p = _fake(pop_mod.PopulationPPO)
    p.envs = [_FakeEnv(), _FakeEnv()]
    p.n_envs = 2
    p._policy_env_step(0)
    assert (p._mlp.fused, p._mlp.plain) == (0, 1) and [e.calls for e in p.envs] == [1, 1]
