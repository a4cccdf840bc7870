"""Host side of the whole-rollout form (kp1_rollout_run) without a GPU: the coverage predicate on plain values, each
trainer's choice of path on fakes, the span split, and the defaults while KP1_ROLLOUT_RUN is unset."""
from __future__ import annotations

import types

import pytest
import torch

from rl_brain_trainer_amd import mlp as kmlp
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import population as kpop
from rl_brain_trainer_amd import ppo as kppo
from rl_brain_trainer_amd.curriculum import PointCurriculum, PointCurriculumPopulation
from rl_brain_trainer_amd.finisher_tools import DockReverseCurriculum
from rl_brain_trainer_amd.route_curriculum import RoutePrefixCurriculumDevice
from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

COVERED = dict(step_covered=True, hidden=64, mode_name="approach", dist_enabled=False, has_step_callback=False, tracker_attached=False,
               envs_per_replica=4096, env_var="1")


def _covered(**kw) -> bool:
    a = {**COVERED, **kw}
    extra = {k: a.pop(k) for k in ("tracker_ok", "default_on") if k in a}
    return kppo.rollout_run_covered(a["step_covered"], a["hidden"], a["mode_name"], a["dist_enabled"], a["has_step_callback"],
                                    a["tracker_attached"], a["envs_per_replica"], a["env_var"], **extra)


# ---------------------------------------------------------------------------------------------------------------- the predicate
def test_predicate_on_plain_values():
    assert _covered() and _covered(hidden=128)
    assert not _covered(step_covered=False)
    assert not _covered(hidden=256) and not _covered(hidden=32)
    assert not _covered(mode_name="dock")
    assert not _covered(dist_enabled=True)
    assert not _covered(has_step_callback=True)
    # a tracker: only while a replica is one 32-row tile, and only the point tracker
    assert _covered(tracker_attached=True, envs_per_replica=32) and _covered(tracker_attached=True, envs_per_replica=1)
    assert not _covered(tracker_attached=True, envs_per_replica=33)
    assert not _covered(tracker_attached=True, envs_per_replica=16, tracker_ok=False)
    assert _covered(tracker_attached=False, envs_per_replica=33, tracker_ok=False)
    assert kppo.ROLLOUT_RUN_TRACKED_MAX_ENVS == 32 and kppo.ROLLOUT_RUN_WIDTHS == (64, 128)


def test_predicate_switch_and_defaults():
    assert not _covered(env_var="0") and not _covered(env_var="0", default_on=True)
    assert _covered(env_var="1") and _covered(env_var="yes")
    assert not _covered(env_var=None)                        # unset: the trainer's default, which is off
    assert _covered(env_var=None, default_on=True)
    assert not _covered(env_var=None, default_on=True, hidden=256)
    assert kppo.ROLLOUT_RUN_ENV == "KP1_ROLLOUT_RUN"
    # no trainer has the new form as its default (not decided by a measurement yet)
    for cls in (kppo.PPO, kpop.ApproachPopulationPPO):
        assert cls.whole_rollout_default is False


# ---------------------------------------------------------------------------------------------------------------- the span split
def test_span_split():
    assert kmlp.span_split(0, 24, 2048) == [(0, 24)]
    assert kmlp.span_split(0, 2048, 2048) == [(0, 2048)]
    assert kmlp.span_split(0, 2049, 2048) == [(0, 2048), (2048, 1)]
    assert kmlp.span_split(5, 20, 8) == [(5, 8), (13, 8), (21, 4)]
    assert kmlp.span_split(3, 1, 1) == [(3, 1)]
    for first, n, cap in ((0, 1, 1), (7, 4097, 2048), (2, 33, 5)):
        spans = kmlp.span_split(first, n, cap)
        assert spans[0][0] == first and sum(c for _, c in spans) == n and all(1 <= c <= cap for _, c in spans)
        assert all(spans[i][0] + spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1))
    with pytest.raises(ValueError):
        kmlp.span_split(0, 0, 8)
    assert native.ROLLOUT_RUN_MAX_STEPS == 2048


def _fake_env(n_envs: int, mode: str = "approach"):
    env = object.__new__(ArmKinematicVecEnv)         # no handle: close() / __del__ find nothing to destroy
    env.n_envs, env.dtype, env._mode_name, env._handle = n_envs, torch.float32, mode, None
    return env


def test_host_split_on_a_fake_library(monkeypatch):
    """MlpKernels.rollout_run over a span above the cap: consecutive kp1_rollout_run calls, each on the buffers from its first slice on"""
    calls = []

    class FakeLib:
        @staticmethod
        def kp1_rollout_run(h, env, obs, stride, noise, value, action, log_prob, reward, done, term, n_steps, trackers, spc, stream):
            calls.append((obs.value, stride, noise.value, None if value is None else value.value, action.value, log_prob, reward.value,
                          done.value, term, n_steps, trackers, spc))
            return 0

    monkeypatch.setattr(native, "ROLLOUT_RUN_MAX_STEPS", 8)
    m = object.__new__(kmlp.MlpKernels)
    m.L, m._h, m._stream = FakeLib, None, (lambda: None)
    T, rows = 20, 3
    env = _fake_env(rows)
    obs = torch.zeros((T + 1, rows, 64))
    noise, action = torch.zeros((T, rows, 7)), torch.zeros((T, rows, 7))
    value, reward, done = torch.zeros((T, rows)), torch.zeros((T, rows)), torch.zeros((T, rows), dtype=torch.uint8)
    m.rollout_run(env, obs, noise=noise, value=value, action=action, log_prob=None, reward=reward, done=done, terminal_obs=None, first_step=0,
                  n_steps=T, steps_per_call=rows)
    assert [c[9] for c in calls] == [8, 8, 4]
    for c, t0 in zip(calls, (0, 8, 16)):
        assert c[0] == obs[t0].data_ptr() and c[2] == noise[t0].data_ptr() and c[3] == value[t0].data_ptr() and c[4] == action[t0].data_ptr()
        assert c[6] == reward[t0].data_ptr() and c[7] == done[t0].data_ptr()
        assert c[1] == 64 and c[5] is None and c[8] is None and c[10] is None and c[11] == rows
    # a span inside the rollout
    calls.clear()
    m.rollout_run(env, obs, noise=noise, value=None, action=action, log_prob=None, reward=reward, done=done, terminal_obs=None, first_step=7,
                  n_steps=13, steps_per_call=rows)
    assert [(c[0], c[9]) for c in calls] == [(obs[7].data_ptr(), 8), (obs[15].data_ptr(), 5)] and calls[0][3] is None
    # route envs (anything that is not an arm env handle) are refused on the host
    with pytest.raises(TypeError, match="route envs"):
        m.rollout_run(types.SimpleNamespace(n_envs=rows), obs, noise=noise, value=None, action=action, log_prob=None, reward=reward, done=done,
                      terminal_obs=None, first_step=0, n_steps=T)


# ---------------------------------------------------------------------------------------------------------------- the trainers' choice
def _fake_ppo(cls, *, hidden=64, n_envs=16, mode="approach", tracker=None, dist_enabled=False, callback=None, population=False):
    p = object.__new__(cls)
    p.cfg = kppo.PPOConfig(n_steps=5, batch_size=16, hidden=hidden)
    p.n_envs, p.obs_dim = n_envs, 56
    p.dist = types.SimpleNamespace(enabled=dist_enabled, world_size=2 if dist_enabled else 1)
    p.step_callback = callback
    env = _fake_env(n_envs, mode)
    if population:
        p.pop_env, p.pop_curriculum = env, tracker
    else:
        p.env, p.curriculum = env, tracker
    return p


def test_ppo_chooses_its_path(monkeypatch):
    point = object.__new__(PointCurriculum)
    monkeypatch.delenv("KP1_ROLLOUT_RUN", raising=False)
    assert not _fake_ppo(kppo.PPO)._whole_rollout                      # unset: off
    monkeypatch.setenv("KP1_ROLLOUT_RUN", "0")
    assert not _fake_ppo(kppo.PPO)._whole_rollout
    monkeypatch.setenv("KP1_ROLLOUT_RUN", "1")
    assert _fake_ppo(kppo.PPO)._whole_rollout
    assert _fake_ppo(kppo.PPO, hidden=128, n_envs=4096)._whole_rollout   # no tracker: any env count
    assert _fake_ppo(kppo.PPO, tracker=point, n_envs=32)._whole_rollout
    assert not _fake_ppo(kppo.PPO, tracker=point, n_envs=40)._whole_rollout
    for other in (RoutePrefixCurriculumDevice, DockReverseCurriculum):              # some other tracker: its own launches
        assert not _fake_ppo(kppo.PPO, tracker=object.__new__(other), n_envs=16)._whole_rollout
    assert not _fake_ppo(kppo.PPO, hidden=256)._whole_rollout
    assert not _fake_ppo(kppo.PPO, mode="dock")._whole_rollout
    assert not _fake_ppo(kppo.PPO, dist_enabled=True)._whole_rollout
    assert not _fake_ppo(kppo.PPO, callback=lambda d: None)._whole_rollout
    p = _fake_ppo(kppo.PPO)
    p.env.dtype = torch.float64
    assert not p._whole_rollout
    p = _fake_ppo(kppo.PPO)
    p.env._reward_components_on = True
    assert not p._whole_rollout
    p = _fake_ppo(kppo.PPO)
    p.env = types.SimpleNamespace(dtype=torch.float32, _mode_name="approach")      # not the plain arm env (a route env, a wrapper)
    assert not p._whole_rollout


def test_populations_choose_their_path(monkeypatch):
    tracker = object.__new__(PointCurriculumPopulation)
    monkeypatch.setenv("KP1_ROLLOUT_RUN", "1")
    assert _fake_ppo(kpop.ApproachPopulationPPO, population=True, tracker=tracker)._whole_rollout
    assert _fake_ppo(kpop.ApproachPopulationPPO, population=True, n_envs=4096)._whole_rollout
    assert not _fake_ppo(kpop.ApproachPopulationPPO, population=True, tracker=tracker, n_envs=33)._whole_rollout
    assert not _fake_ppo(kpop.ApproachPopulationPPO, population=True, callback=lambda d: None)._whole_rollout
    # the K-handle population and the dock / route one-handle populations keep the per-step loop whatever the switch says
    for cls in (kpop.PopulationPPO, kpop.DockPopulationPPO, kpop.RoutePopulationPPO):
        assert _fake_ppo(cls, population=True)._whole_rollout is False
    monkeypatch.delenv("KP1_ROLLOUT_RUN")
    assert not _fake_ppo(kpop.ApproachPopulationPPO, population=True)._whole_rollout


@pytest.mark.parametrize("form", ["1", "0", None])
def test_collect_rollouts_takes_the_chosen_path(form, monkeypatch):
    """eager collect_rollouts on a fake: one _rollout_whole call, or n_steps per-step calls, then the unchanged _post_rollout"""
    if form is None:
        monkeypatch.delenv("KP1_ROLLOUT_RUN", raising=False)
    else:
        monkeypatch.setenv("KP1_ROLLOUT_RUN", form)
    p = _fake_ppo(kppo.PPO)
    seen = []
    p._needs_reset, p.use_graphs, p.num_timesteps, p._kernels_warm = False, False, 0, False
    p.obs_buf = torch.zeros((6, 16, 64))
    p._draw_noise = lambda: seen.append("noise")
    p._rollout_whole = lambda *a, **k: seen.append("whole")
    p._rollout_step_hip = lambda t: seen.append(("step", t))
    p._post_rollout = lambda: seen.append("post")
    p.collect_rollouts()
    if form == "1":
        assert seen == ["noise", "whole", "post"]
    else:
        assert seen == ["noise"] + [("step", t) for t in range(5)] + ["post"]
    assert p.num_timesteps == 5 * 16
