"""The host side of the one-launch route rollout step without a GPU: the symbol is declared, exported and bound, the waypoint limit of the header
equals the Python constant, the predicate that chooses the form (ppo.fused_route_rollout_covered) on plain values, and which path
RoutePopulationPPO and PPO take, on fakes."""
from __future__ import annotations

import re

import pytest
import torch

from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import population as pop_mod
from rl_brain_trainer_amd import ppo as ppo_mod
from rl_brain_trainer_amd.ppo import PPOConfig, fused_rollout_covered, fused_route_rollout_covered

F32, F64 = torch.float32, torch.float64
SYMBOL = "kp1_mlp_forward_route_step"


def test_symbol_declared_exported_and_bound():
    assert SYMBOL in native.declared_symbols()
    L = native.load()
    fn = getattr(L, SYMBOL)                      # exported by libkp1.so
    assert fn.argtypes is not None and len(fn.argtypes) == 13      # bound by native.load()
    header = (kcfg.repo_root() / "include" / "kp1_route.h").read_text()
    assert "struct kp1_mlp;" in header           # the header stays self-contained


def test_waypoint_limit_matches_the_header():
    header = (kcfg.repo_root() / "include" / "kp1_route.h").read_text()
    m = re.search(r"#define\s+KP1_ROUTE_FUSED_MAX_WAYPOINTS\s+(\d+)", header)
    assert m and int(m.group(1)) == ppo_mod.ROUTE_FUSED_MAX_WAYPOINTS
    # the x + h1 tiles of the 64-column kernel, 32 rows at pitches 68 and 132, hold the [W][7] joint table
    assert ppo_mod.ROUTE_FUSED_MAX_WAYPOINTS == (32 * 68 + 32 * 132) // 7


def _covered(env_type_ok=True, dtype=F32, hidden=64, obs_dim=80, components_on=False, n_waypoints=484, dist_enabled=False, env_var="1"):
    return fused_route_rollout_covered(env_type_ok, dtype, hidden, obs_dim, components_on, n_waypoints, dist_enabled, env_var)


def test_predicate_on_plain_values():
    for hidden in (64, 128):
        for obs_dim in (56, 80):
            assert _covered(hidden=hidden, obs_dim=obs_dim)
    assert _covered(env_var="yes")
    assert not _covered(env_var=None)            # opt-in: unset is the launch sequence
    assert not _covered(env_var="0")
    assert not _covered(env_type_ok=False)
    assert not _covered(dtype=F64)
    assert not _covered(hidden=256)
    assert not _covered(hidden=32)
    assert not _covered(obs_dim=64)              # the observation width, not the pitch
    assert not _covered(components_on=True)      # recorded reward components fall back
    assert not _covered(dist_enabled=True)       # data-parallel runs fall back
    assert _covered(n_waypoints=ppo_mod.ROUTE_FUSED_MAX_WAYPOINTS)
    assert not _covered(n_waypoints=ppo_mod.ROUTE_FUSED_MAX_WAYPOINTS + 1)


def test_the_arm_switch_alone_never_selects_the_route_form(monkeypatch):
    """KP1_FUSED_ROLLOUT is the arm envs' variable: the route form answers to KP1_FUSED_ROUTE_ROLLOUT only, and the arm predicate keeps
    refusing the 80-float observation"""
    assert ppo_mod.FUSED_ROUTE_ROLLOUT_ENV == "KP1_FUSED_ROUTE_ROLLOUT"
    assert not fused_rollout_covered(True, F32, 64, 80, False, "1")
    monkeypatch.setenv("KP1_FUSED_ROLLOUT", "1")
    monkeypatch.delenv("KP1_FUSED_ROUTE_ROLLOUT", raising=False)
    p = _fake_population()
    assert not p._fused_route_step
    p._policy_env_step(0)
    assert (p._mlp.route, p._mlp.fused, p._mlp.plain, p.pop_env.calls) == (0, 0, 1, 1)


class _Dist:
    def __init__(self, enabled: bool = False) -> None:
        self.enabled = enabled


class _FakeEnv:
    """what a trainer reads of a route env once the switch is set"""
    dtype = F32

    def __init__(self, components: bool = False, n_waypoints: int = 484) -> None:
        self._reward_components_on = components
        self.n_waypoints = n_waypoints
        self.calls = 0

    def step_into(self, *args) -> None:
        self.calls += 1


class _BareEnv:
    """a fake without any of the attributes the route predicate reads: the unset switch must not touch them"""
    dtype = F32

    def __init__(self) -> None:
        self.calls = 0

    def step_into(self, *args) -> None:
        self.calls += 1


class _FakeMlp:
    def __init__(self) -> None:
        self.route, self.fused, self.plain = 0, 0, 0

    def forward_route_step(self, env, obs, **kw) -> None:
        assert set(kw) == {"noise", "value", "action", "log_prob", "next_obs", "reward", "done", "terminal_obs"}
        self.route += 1

    def forward_env_step(self, env, obs, **kw) -> None:
        self.fused += 1

    def forward(self, obs, **kw) -> None:
        self.plain += 1


def _buffers(p) -> None:
    for name in ("obs_buf", "noise_all", "val_buf", "act_buf", "logp_buf", "rew_buf", "done_buf", "term_obs_buf"):
        setattr(p, name, torch.zeros((3, 4, 1)))
    p.clip_act = torch.zeros((4, 7))


def _fake_population(cls=None, *, env=None, hidden: int = 64, obs_dim: int = 80, dist: bool = False):
    p = object.__new__(cls or pop_mod.RoutePopulationPPO)
    p.cfg = PPOConfig(n_steps=2, hidden=hidden)
    p.obs_dim = obs_dim
    p.pop_env = env if env is not None else _FakeEnv()
    p.dist = _Dist(dist)
    p._mlp = _FakeMlp()
    _buffers(p)
    return p


@pytest.mark.parametrize("env_var,want", [("1", True), ("0", False), (None, False)])
def test_route_population_chooses_the_path(env_var, want, monkeypatch):
    monkeypatch.delenv("KP1_FUSED_ROLLOUT", raising=False)
    if env_var is None:
        monkeypatch.delenv("KP1_FUSED_ROUTE_ROLLOUT", raising=False)
    else:
        monkeypatch.setenv("KP1_FUSED_ROUTE_ROLLOUT", env_var)
    for obs_dim in (56, 80):
        p = _fake_population(obs_dim=obs_dim)
        p._policy_env_step(0)
        assert (p._mlp.route, p._mlp.fused, p._mlp.plain, p.pop_env.calls) == ((1, 0, 0, 0) if want else (0, 0, 1, 1)), (env_var, obs_dim)


def test_route_population_falls_back(monkeypatch):
    monkeypatch.setenv("KP1_FUSED_ROUTE_ROLLOUT", "1")
    for kw in ({"env": _FakeEnv(components=True)}, {"env": _FakeEnv(n_waypoints=ppo_mod.ROUTE_FUSED_MAX_WAYPOINTS + 1)}, {"hidden": 256},
               {"dist": True}):
        p = _fake_population(**kw)
        p._policy_env_step(0)
        assert (p._mlp.route, p._mlp.plain, p.pop_env.calls) == (0, 1, 1), kw
    # the component switch is read at every step: thrown after construction, the next step falls back
    p = _fake_population()
    p._policy_env_step(0)
    p.pop_env._reward_components_on = True
    p._policy_env_step(1)
    assert (p._mlp.route, p._mlp.plain, p.pop_env.calls) == (1, 1, 1)


def test_other_one_handle_populations_never_take_the_route_form(monkeypatch):
    monkeypatch.setenv("KP1_FUSED_ROUTE_ROLLOUT", "1")
    monkeypatch.setenv("KP1_FUSED_ROLLOUT", "0")
    for name in ("ApproachPopulationPPO", "DockPopulationPPO", "OneHandlePopulationPPO"):
        p = _fake_population(getattr(pop_mod, name), obs_dim=56)
        p._policy_env_step(0)
        assert (p._mlp.route, p._mlp.fused, p._mlp.plain, p.pop_env.calls) == (0, 0, 1, 1), name


def test_unset_switch_reads_nothing_of_the_env(monkeypatch):
    """no variable set: RoutePopulationPPO takes forward + step_into on an env that lacks every attribute the route predicate reads"""
    monkeypatch.delenv("KP1_FUSED_ROUTE_ROLLOUT", raising=False)
    monkeypatch.delenv("KP1_FUSED_ROLLOUT", raising=False)
    p = _fake_population(env=_BareEnv())
    del p.dist
    p._policy_env_step(0)
    assert (p._mlp.route, p._mlp.fused, p._mlp.plain, p.pop_env.calls) == (0, 0, 1, 1)


def _fake_ppo(env, *, hidden: int = 64, obs_dim: int = 80, dist: bool = False):
    p = object.__new__(ppo_mod.PPO)
    p.env, p.cfg, p.obs_dim, p.dist = env, PPOConfig(n_steps=2, hidden=hidden), obs_dim, _Dist(dist)
    p._mlp = _FakeMlp()
    _buffers(p)
    return p


def _route_env(cls, components: bool = False):
    env = object.__new__(cls)
    env.dtype, env.n_waypoints, env._reward_components_on, env.calls = F32, 484, components, 0
    env._handle = None      # (nothing to close)
    env.step_into = lambda *args: setattr(env, "calls", env.calls + 1)
    return env


def test_single_seed_ppo_chooses_the_path(monkeypatch):
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv, RouteVecEnv
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    monkeypatch.delenv("KP1_FUSED_ROLLOUT", raising=False)
    monkeypatch.setenv("KP1_FUSED_ROUTE_ROLLOUT", "1")
    env = _route_env(RouteVecEnv)
    p = _fake_ppo(env)
    p._policy_env_step(0)
    assert (p._mlp.route, p._mlp.fused, p._mlp.plain, env.calls) == (1, 0, 0, 0)
    env._reward_components_on = True            # thrown after construction
    p._policy_env_step(1)
    assert (p._mlp.route, p._mlp.plain, env.calls) == (1, 1, 1)
    for kw in ({"hidden": 256}, {"dist": True}):
        env = _route_env(RouteVecEnv)
        p = _fake_ppo(env, **kw)
        p._policy_env_step(0)
        assert (p._mlp.route, p._mlp.plain, env.calls) == (0, 1, 1), kw
    # PPO steps single handles: a population route env is RoutePopulationPPO's; an arm env keeps its own switch
    assert not _fake_ppo(_route_env(RoutePopulationVecEnv))._fused_route_step
    arm = object.__new__(ArmKinematicVecEnv)
    arm.dtype, arm._handle = F32, None
    assert not _fake_ppo(arm, obs_dim=56)._fused_route_step
    # unset: the launch sequence
    monkeypatch.delenv("KP1_FUSED_ROUTE_ROLLOUT")
    env = _route_env(RouteVecEnv)
    p = _fake_ppo(env)
    p._policy_env_step(0)
    assert (p._mlp.route, p._mlp.fused, p._mlp.plain, env.calls) == (0, 0, 1, 1)


def test_train_route_flag_sets_the_switch():
    from rl_brain_trainer_amd import train_route

    args = train_route.build_arg_parser().parse_args(["--config", "x.yaml", "--run-id", "r", "--seed", "1", "--one-launch-rollout"])
    assert args.one_launch_rollout
    assert not train_route.build_arg_parser().parse_args(["--config", "x.yaml", "--run-id", "r", "--seed", "1"]).one_launch_rollout
