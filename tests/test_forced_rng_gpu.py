"""The RNG restatement's rare branches, forced on purpose, in every kernel the reset samplers are compiled into (GPU part).

Each test builds one handle of N = 130 envs (two full waves and a ragged one), gives every env its own PCG64 state through set_rng_state --
the forced rows of one group of tests/golden/forced_rng_resets.npz interleaved with ordinary seeds, so that every wave mixes lanes on the
rare branches with lanes on the fast path -- and compares what the kernel's sampler left with the CPU oracle run from the same words: the
words after, the integer fields and the sampled state.  fp64 handles bit for bit; fp32 handles words and integers bit for bit and floats
as test_reset_stream_gpu / test_route_env_f32_gpu compare them (q = the two-float rounding of the fp64 draw, the other planes its fp32
rounding).  The rows that come from the fixture are also compared with the reference's recorded values.  Which classes a batch holds is
established on the CPU (rng_forcing.classify on numpy's Generator, the oracle's word counts) before anything is launched, and printed.

The step kernels resample inside the launch: the configs run episodes of one step, so the step after set_rng_state truncates every env and
its auto-reset draws from the forced words (the reset does not depend on the action)."""
from __future__ import annotations

import json
from functools import lru_cache

import numpy as np
import pytest
import torch

import rng_forcing as rf
from conftest import GOLDEN
from oracle import oracle as orc
from oracle import route_oracle as ro
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import route_config as rcfg
from test_env_parity_gpu import F32_POSE_TOL, F64_TOL, _two_float
from test_forced_rng_cpu import classes_in, fixture, group_cfg_dict, rows_of, set_oracle_rng

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N = 130
# episodes of one step that always end by truncation: a route env that starts on its waypoint (recovery resets) would otherwise meet the base
# env's success test at once, which ends no episode of a sequence env
ONE_STEP = {"env.termination.max_episode_steps": 1, "env.episode_length": 1, "env.termination.terminate_on_success": False}
ZIGGURAT = ("wedge_accept", "wedge_reject", "tail", "tail_retry")
GROUPS = sorted(fixture()["groups"])


# ============================================================================== the batch and its oracle (CPU only)
def _configs(group: str):
    cfgd = group_cfg_dict(group, ONE_STEP)
    base = kcfg.to_env_config(cfgd, handoff_base_dirs=(GOLDEN,))
    return cfgd, base


@lru_cache(maxsize=None)
def _route_q() -> np.ndarray:
    return rcfg.load_route_q(GOLDEN / "synthetic_route.json")


def _route_draws(group: str, mode: int) -> list:
    """the draw sequence of one route reset of the group's config in reset mode `mode`"""
    r = rcfg.route_config_from_dict(group_cfg_dict(group)).reset
    W = min(int(r.max_route_index), _route_q().shape[0] - 1)
    hi = {2: min(int(r.segment_end_index), W), 3: min(int(r.replay_end_index), W)}.get(mode, W)
    lo = {2: int(r.segment_start_index), 3: int(r.replay_start_index)}.get(mode, int(r.min_route_index))
    normals = 7 * sum(float(v) > 0.0 for v in (r.q_noise_std, r.dq_noise_std, r.prev_action_noise_std))
    return ["double", ("integers", lo, hi + 1)] + ["normal"] * normals


class Batch:
    """N states of one group (forced fixture rows two lanes in three, or every other lane, ordinary seeds between them), the oracle's reset
    of each (`resets` consecutive resets: the state after the last one, the words after each), and the classes present, verified on the CPU"""

    def __init__(self, group: str, *, resets: int = 1, seed0: int = 70000) -> None:
        f = fixture()
        self.group, self.kind = group, f["groups"][group]["kind"]
        self.stage = int(f["groups"][group]["stage"])
        forced = list(rows_of(group))
        period = 2 if len(forced) <= N // 2 else 3
        slots = np.array([i for i in range(N) if i % period != 0])      # every other lane, or two in three, up to the ragged last wave
        assert len(forced) <= slots.size and slots[-1] >= 128
        lanes = slots[np.round(np.linspace(0, slots.size - 1, len(forced))).astype(int)]      # spread evenly, the last row in the last wave
        assert np.unique(lanes).size == len(forced)
        self.row = np.full(N, -1, dtype=np.int64)           # fixture row of lane i, or -1: ordinary seed
        self.row[lanes] = forced
        self.words = np.array([f["words_before"][self.row[i]] if self.row[i] >= 0 else rf.seed_words(seed0 + i) for i in range(N)], dtype=np.uint64)
        self._oracle(resets)
        self._classes()

    def _oracle(self, resets: int) -> None:
        cfgd, base = _configs(self.group)
        self.ref = {k: np.zeros((N, 6 if k == "goal_pose6" else 7)) for k in ("q", "dq", "prev_action", "goal_q", "goal_pose6")}
        self.ints = np.full((N, 4), -1, dtype=np.int64)      # route_index, start_route_index, reset_mode, stage
        self.after = np.zeros((resets, N, 6), dtype=np.uint64)
        self.first_ints = np.full((N, 4), -1, dtype=np.int64)
        if self.kind == "route":
            L = ro.lib()
            env = ro.OracleRouteEnv(base, rcfg.route_config_from_dict(cfgd), ro.Route(_route_q()))
            for i in range(N):
                set_oracle_rng(L.kp1o_route_env_rng(env._p).contents, self.words[i])
                for r in range(resets):
                    env.reset()
                    self.after[r, i] = env.rng_words()
                    ints = [env.field("current_route_index"), env.field("start_route_index"), env.field("reset_mode"), -1]
                    if r == 0:
                        self.first_ints[i] = ints
                self.ints[i] = ints
                st = env.base_state()
                for k in self.ref:
                    self.ref[k][i] = st[k]
        else:
            env = orc.OracleEnv(base)
            env.set_curriculum_stage(self.stage)
            for i in range(N):
                set_oracle_rng(env.e.rng, self.words[i])
                for r in range(resets):
                    env.reset()
                    self.after[r, i] = env.rng_words()
                    if r == 0:
                        self.first_ints[i, 3] = int(env.e.last_reset_stage)
                self.ints[i, 3] = int(env.e.last_reset_stage)
                st = env.state()
                for k in self.ref:
                    self.ref[k][i] = st[k]

    def _classes(self) -> None:
        """what the batch holds, decided by numpy's Generator and the oracle's word counts alone"""
        f = fixture()
        found: dict[str, int] = {}
        for i in np.flatnonzero(self.row >= 0):
            j, w = self.row[i], self.words[i]
            cls = str(f["cls"][j])
            if f["u_k"][j] >= 0:
                assert rf.generator_of(w).random() == int(f["u_k"][j]) * 2.0 ** -53
            classes_in(w, json.loads(str(f["draws"][j])), json.loads(str(f["expect"][j])))
            if cls in ("rot0", "rot63"):
                bg = rf.bitgen_of(w)
                bg.random_raw()
                assert int(rf.words_of(bg)[0]) >> 58 == (0 if cls == "rot0" else 63)
            assert rf.lcg_steps(w, self.after[0, i]) == int(f["words_used"][j]), (self.group, str(f["label"][j]))   # the config-forced loops
            found[cls] = found.get(cls, 0) + 1
        self.classes = found
        self.fast_lanes = np.zeros(N, dtype=bool)
        if self.kind == "route":     # lanes whose whole reset stays on the fast paths
            for i in range(N):
                labels = [lab for lab, _ in rf.classify(self.words[i], _route_draws(self.group, int(self.first_ints[i, 2])))]
                self.fast_lanes[i] = all(lab in ("double", "integers", "fast") for lab in labels)
            for i in np.flatnonzero(self.row >= 0):
                if f["cls"][self.row[i]] in ZIGGURAT + ("lemire_zero", "lemire_reject"):   # a rare lane with fast lanes in its wave
                    wave = slice(i // 64 * 64, min(i // 64 * 64 + 64, N))
                    assert self.fast_lanes[wave].any() and not self.fast_lanes[i], (self.group, i)
        else:
            self.fast_lanes[self.row < 0] = True

    def describe(self, kernel: str, real: str) -> str:
        waves = [sorted({str(fixture()["cls"][j]) for j in self.row[w:w + 64] if j >= 0}) for w in range(0, N, 64)]
        return (f"\n[{kernel}] {self.group} {real}: {int(np.sum(self.row >= 0))} forced lanes of {N}; classes {json.dumps(self.classes, sort_keys=True)}; "
                f"rare classes per wave {[len(w) for w in waves]}; lanes wholly on the fast paths {int(self.fast_lanes.sum())}")

    def require(self, *classes: str) -> None:
        for c in classes:
            assert self.classes.get(c, 0) >= 1, (self.group, c, self.classes)

    # ---- the comparison
    def check(self, ctx, *, real: str, words: np.ndarray, state: dict, stage: np.ndarray | None = None, route: dict | None = None, last: int = 0,
              against_fixture: bool = True) -> None:
        bad = np.flatnonzero(np.any(words != self.after[last], axis=1))
        assert bad.size == 0, (ctx, "words after", bad[:8], [str(fixture()["label"][j]) if j >= 0 else "seed" for j in self.row[bad[:8]]])
        if route is not None:
            for col, key in enumerate(("route_index", "start_route_index", "route_reset_mode")):
                assert np.array_equal(route[key], self.ints[:, col]), (ctx, key, np.flatnonzero(route[key] != self.ints[:, col])[:8])
        if stage is not None:
            assert np.array_equal(stage, self.ints[:, 3]), (ctx, "stage", np.flatnonzero(stage != self.ints[:, 3])[:8])
        cast = (lambda x: x) if real == "f64" else (lambda x: x.astype(np.float32).astype(np.float64))
        assert np.array_equal(state["q"], self.ref["q"] if real == "f64" else _two_float(self.ref["q"])), (ctx, "q")
        for k in ("dq", "prev_action", "goal_q"):
            assert np.array_equal(state[k], cast(self.ref[k])), (ctx, k, np.flatnonzero(np.any(state[k] != cast(self.ref[k]), axis=1))[:8])
        assert np.max(np.abs(state["goal_pose6"] - self.ref["goal_pose6"])) <= (F64_TOL if real == "f64" else F32_POSE_TOL), (ctx, "goal_pose6")
        if not against_fixture or last != 0:
            return
        f = fixture()          # the reference's own record of the forced rows
        lanes = np.flatnonzero(self.row >= 0)
        rows = self.row[lanes]
        assert np.array_equal(words[lanes], f["words_after"][rows]), (ctx, "fixture words")
        for dev_key, fix_key in (("q", "initial_q"), ("dq", "initial_dq"), ("prev_action", "initial_prev_action")):
            want = f[fix_key][rows]
            want = want if real == "f64" else (_two_float(want) if dev_key == "q" else cast(want))
            assert np.array_equal(state[dev_key][lanes], want), (ctx, "fixture", fix_key)
        if self.kind == "route":
            for col, key in enumerate(("route_index", "start_route_index", "route_reset_mode")):
                assert np.array_equal(route[key][lanes], f["ints"][rows, col]), (ctx, "fixture", key)
        else:
            assert np.array_equal(state["goal_q"][lanes], cast(f["goal_q"][rows])), (ctx, "fixture goal_q")
            known = f["ints"][rows, 3] >= 0
            assert np.array_equal(stage[lanes][known], f["ints"][rows, 3][known]), (ctx, "fixture stage")


@lru_cache(maxsize=None)
def _batch(group: str, resets: int = 1) -> Batch:
    """computed once per group and shared; nothing modifies it"""
    return Batch(group, resets=resets)


# ============================================================================== handles
def _make_env(group: str, real: str, *, pitch: int | None = None):
    from rl_brain_trainer_amd.route_env import RouteVecEnv
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    cfgd, base = _configs(group)
    g = fixture()["groups"][group]
    if g["kind"] == "route":
        env = RouteVecEnv(base, rcfg.route_config_from_dict(cfgd), _route_q(), N, seed=5, real=real)
    else:
        env = ArmKinematicVecEnv(base, N, seed=5, real=real)
        env.set_curriculum_stage(int(g["stage"]))
    if pitch is not None:
        env.set_obs_stride(pitch)
    return env


def _read(env) -> dict:
    torch.cuda.synchronize()
    info = env.info()
    out = {"words": env.rng_state(), "state": env.get_state(), "stage": info["stage_index"].cpu().numpy().astype(np.int64), "route": None}
    if "route_index" in info:
        out["route"] = {k: info[k].cpu().numpy().astype(np.int64) for k in ("route_index", "start_route_index", "route_reset_mode")}
        out["stage"] = None
    return out


def _check_env(b: Batch, env, ctx, real: str, *, last: int = 0) -> None:
    r = _read(env)
    b.check(ctx, real=real, words=r["words"], state=r["state"], stage=r["stage"], route=r["route"], last=last)


def _announce(capsys, text: str) -> None:
    """the classes of the batch, in the test's output whether or not pytest captures it"""
    with capsys.disabled():
        print(text)


def _far_action(dtype) -> torch.Tensor:
    """full-scale actions (the state a reset samples does not depend on the action)"""
    return torch.ones((N, 7), dtype=dtype, device=DEV)


def _far_noise(shape) -> torch.Tensor:
    """the same through a policy: four standard deviations on every joint (the test policies' log_std is near -1: the clipped action is 1)"""
    return torch.full(shape, 4.0, dtype=torch.float32, device=DEV)


def _all_done(done: torch.Tensor, ctx) -> None:
    assert bool((done & 3).ne(0).all()), (ctx, "an env did not finish its one-step episode")


# ============================================================================== 1. the stand-alone reset kernels and the step kernels
@pytest.mark.parametrize("real", ["f64", "f32"])
@pytest.mark.parametrize("group", GROUPS)
def test_reset_and_step_kernels(group, real, capsys):
    """kp1_route_reset_kernel / kp1_reset_kernel (explicit sampled reset) and the auto-reset of kp1_route_step_kernel / kp1_step_kernel, approach
    and dock modes, on every group of the fixture"""
    b = _batch(group)
    kind = fixture()["groups"][group]["kind"]
    names = ("kp1_route_reset_kernel", "kp1_route_step_kernel") if kind == "route" else ("kp1_reset_kernel", "kp1_step_kernel")
    _announce(capsys, b.describe(" + ".join(names), real))
    if group == "route170":
        b.require(*ZIGGURAT, "lemire_zero", "lemire_reject", "lemire_at_threshold", "u_boundary", "rot0", "rot63")
    env = _make_env(group, real)
    env.reset()
    env.set_rng_state(b.words)
    env.reset()
    _check_env(b, env, (group, real, names[0]), real)
    env.set_rng_state(b.words)
    _, _, done = env.step(_far_action(env.dtype))
    _all_done(done, (group, real))
    _check_env(b, env, (group, real, names[1]), real)
    env.close()


# ============================================================================== 2. the one-launch rollout steps
@pytest.mark.parametrize("group", ["route170", "route120"])
@pytest.mark.parametrize("hidden", [64, 128])
def test_route_rollout_step_kernel(hidden, group, capsys):
    """route_rollout_step_kernel: the policy forward of a row tile and the route step of its envs, auto-reset included, in one launch"""
    from test_route_rollout_step_gpu import _mlp

    b = _batch(group)
    _announce(capsys, b.describe(f"route_rollout_step_kernel hidden {hidden}", "f32"))
    b.require("lemire_reject", "u_boundary", "rot63", *(ZIGGURAT if group == "route170" else ()))
    env = _make_env(group, "f32", pitch=128)
    assert env.obs_dim == 80
    mlp = _mlp(hidden, 1, 80, seed=hidden, max_batch=256)
    obs = env.reset().clone()
    env.set_rng_state(b.words)
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=DEV)   # noqa: E731
    done = z(N, dt=torch.uint8)
    noise = _far_noise((N, 7))
    mlp.forward_route_step(env, obs, noise=noise, value=z(N), action=z(N, 7), log_prob=z(N), next_obs=z(N, 128), reward=z(N), done=done,
                           terminal_obs=z(N, 128))
    _all_done(done, (group, hidden))
    _check_env(b, env, (group, hidden, "route_rollout_step_kernel"), "f32")
    mlp.close()
    env.close()


@pytest.mark.parametrize("group", ["ws9", "rs10", "rs10_mid", "dock_handoff", "dock_later"])
@pytest.mark.parametrize("hidden", [64, 128])
def test_rollout_step_kernel(hidden, group, capsys):
    """rollout_step_kernel (kp1_mlp_forward_env_step on a hidden 64 / 128 handle), approach and dock modes"""
    from test_rollout_step_layerwise_gpu import _mlp

    b = _batch(group)
    _announce(capsys, b.describe(f"rollout_step_kernel hidden {hidden}", "f32"))
    env = _make_env(group, "f32", pitch=64)
    mlp, _ = _mlp(hidden, 1, 256, seed=hidden)
    obs = env.reset().clone()
    env.set_rng_state(b.words)
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=DEV)   # noqa: E731
    done = z(N, dt=torch.uint8)
    noise = torch.randn((N, 7), generator=torch.Generator(device=DEV).manual_seed(4), device=DEV)
    mlp.forward_env_step(env, obs, noise=noise, value=z(N), action=z(N, 7), log_prob=z(N), next_obs=z(N, 64), reward=z(N), done=done,
                         terminal_obs=z(N, 64))
    _all_done(done, (group, hidden))
    _check_env(b, env, (group, hidden, "rollout_step_kernel"), "f32")
    mlp.close()
    env.close()


# ============================================================================== 3. the whole-rollout kernel
@pytest.mark.parametrize("hidden,group", [(64, "rs10"), (128, "ws9"), (64, "rs10_far")])
def test_rollout_run_kernel(hidden, group, capsys):
    """rollout_run_kernel over a span of 2 steps: both steps end the one-step episodes, so every env resamples twice inside the launch -- from
    the forced words, then from the words that reset left.  The state after the second reset and the words after it are the oracle's; the
    words can only agree if the first reset consumed what the oracle's did."""
    from test_rollout_run_gpu import _buffers, _mlp, _noise

    b = _batch(group, 2)
    _announce(capsys, b.describe(f"rollout_run_kernel hidden {hidden}, 2 steps", "f32"))
    env = _make_env(group, "f32", pitch=64)
    mlp = _mlp(hidden, 1, seed=hidden, max_batch=256)
    buf = _buffers(2, N, 64)
    noise = _noise(2, N, 5)
    buf["obs"][0].copy_(env.reset())
    env.set_rng_state(b.words)
    mlp.rollout_run(env, buf["obs"], noise=noise, value=buf["value"], action=buf["action"], log_prob=buf["log_prob"], reward=buf["reward"],
                    done=buf["done"], terminal_obs=buf["terminal_obs"], first_step=0, n_steps=2, trackers=None, steps_per_call=N)
    torch.cuda.synchronize()
    _all_done(buf["done"][0], (group, hidden, 0))
    _all_done(buf["done"][1], (group, hidden, 1))
    _check_env(b, env, (group, hidden, "rollout_run_kernel"), "f32", last=1)
    mlp.close()
    env.close()


# ============================================================================== 4. the dock population handle (LIVE sampler)
@pytest.mark.parametrize("group", ["dock_handoff", "dock_never", "dock_later"])
def test_dock_population_live_sampler(group, capsys):
    """K = 2 replicas of 65 envs with a one-stage DockReverseCurriculumPopulation attached: reset and step sample with each replica's live
    stage record (the LIVE form of the sampler), which holds the config's own values -- so the oracle of the plain config applies"""
    from rl_brain_trainer_amd import finisher_tools as ft
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    b = _batch(group)
    _announce(capsys, b.describe("kp1_reset_kernel + kp1_step_kernel, dock population K = 2 (LIVE sampler)", "f32"))
    _, base = _configs(group)
    env = ArmKinematicPopulationVecEnv(base, [5, 900], N // 2, mode="dock")
    cur = ft.DockReverseCurriculumPopulation(stages=[{"name": "only"}], window_episodes=4, n_replicas=2, handoff_base_dirs=(GOLDEN,))
    cur.attach(env)
    env.reset()
    env.set_rng_state(b.words)
    env.reset()
    _check_env(b, env, (group, "population reset"), "f32")
    env.set_rng_state(b.words)
    _, _, done = env.step(_far_action(torch.float32))
    _all_done(done, group)
    _check_env(b, env, (group, "population step"), "f32")
    cur.close()
    env.close()
