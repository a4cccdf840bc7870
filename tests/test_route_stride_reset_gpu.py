"""Route-stride Approach resets (env.route_reset) in every kernel that inlines the reset sampler (GPU part).

The yardstick is the reference's own record (tests/golden/route_stride_resets.npz and the trace next to it, made by
make_golden_route_stride_reset.py) and, on the lanes that carry ordinary seeds, the numpy restatement tests/route_stride_reset.py, which
test_route_stride_reset_cpu.py pins to that record bit for bit.  goal_pose6 and the first observation of a sampled pair come from the CPU
oracle's explicit reset (reset(options={initial_q, goal_q}): its FK and observation builder, which its own tests pin to the reference).

Handles hold N = 130 envs (two full waves and a ragged one): the fixture rows of one group and stage spread between ordinary-seed lanes
through set_rng_state, as test_forced_rng_gpu.py does.  Tolerances are test_reset_stream_gpu's: fp64 handles bit for bit on the words, q,
goal_q, dq and prev_action, F64_TOL on goal_pose6 and 6e-8 on the observation; fp32 handles bit for bit on the words, q as the two-float
rounding, the other planes as the fp32 rounding, F32_POSE_TOL on goal_pose6 and 2e-6 on the observation."""
from __future__ import annotations

import json
from functools import lru_cache

import numpy as np
import pytest
import torch

import rng_forcing as rf
from conftest import GOLDEN
from oracle import oracle as orc
from rl_brain_trainer_amd import config as kcfg
from test_env_parity_gpu import F32_POSE_TOL, F64_TOL, _two_float
from test_oracle_golden import TRACES, ref_obs_to_kp1
from test_route_stride_reset_cpu import SCENE, fixture, group_cfg_dict, restate, rows_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N = 130
ONE_STEP = {"env.termination.max_episode_steps": 1, "env.episode_length": 1, "env.termination.terminate_on_success": False}
# (group, stage) of every family of rows in the fixture
CASES = [("scene", 0), ("scene", 3), ("scene", 5), ("scene_fixed", 0), ("tiny_nodraw", 0), ("tiny_nodraw", 1), ("tiny_nodraw", 2),
         ("tiny_reverse", 0), ("tiny_clip", 0), ("tiny_rev8", 1)]


def _env_config(group: str, extra: dict | None = None) -> kcfg.EnvConfig:
    return kcfg.to_env_config(group_cfg_dict(group, extra), handoff_base_dirs=(GOLDEN,))


# ============================================================================== the batch and its reference (CPU only)
class Batch:
    """N states of one (group, stage): up to 64 fixture rows on every other lane, ordinary seeds between them; `resets` consecutive resets of
    each by the restatement (words after each, the pair of the last), and the oracle's goal pose and observation of that pair"""

    def __init__(self, group: str, stage: int, resets: int = 1, seed0: int = 81000) -> None:
        f = fixture()
        self.group, self.stage = group, stage
        rows = rows_of(group, stage)
        forced = rows[f["cls"][rows] != "stream"]
        stream = rows[f["cls"][rows] == "stream"]
        rows = np.concatenate([forced, stream])[:64]           # the forced classes first, then the head of the consecutive stream
        assert rows.size >= 2
        slots = np.arange(1, N, 2)
        lanes = slots[np.round(np.linspace(0, slots.size - 1, rows.size)).astype(int)]     # spread evenly, the last row in the ragged wave
        assert np.unique(lanes).size == rows.size and lanes[-1] >= 128
        self.row = np.full(N, -1, dtype=np.int64)
        self.row[lanes] = rows
        self.words = np.array([f["words_before"][self.row[i]] if self.row[i] >= 0 else rf.seed_words(seed0 + i) for i in range(N)], dtype=np.uint64)
        self.after = np.zeros((resets, N, 6), dtype=np.uint64)
        self.q, self.goal_q = np.zeros((N, 7)), np.zeros((N, 7))
        for i in range(N):
            w = self.words[i]
            for r in range(resets):
                s = restate(group, stage, w)
                w = self.after[r, i] = s["words_after"]
            self.q[i], self.goal_q[i] = s["initial_q"], s["goal_q"]
        env = orc.OracleEnv(_env_config(group, ONE_STEP))
        self.goal_pose6, self.obs = np.zeros((N, 6)), np.zeros((N, kcfg.OBS_DIM), dtype=np.float32)
        for i in range(N):
            self.obs[i] = env.reset(options={"initial_q": self.q[i], "goal_q": self.goal_q[i]})
            st = env.state()
            assert np.array_equal(st["q"], self.q[i]) and np.array_equal(st["goal_q"], self.goal_q[i])      # inside the limits already: not clipped again
            self.goal_pose6[i] = st["goal_pose6"]
        if resets == 1:          # the oracle's pose and observation against the reference's record
            lanes = np.flatnonzero(self.row >= 0)
            assert np.max(np.abs(self.goal_pose6[lanes] - f["goal_pose6"][self.row[lanes]])) <= 1e-12
            assert np.max(np.abs(self.obs[lanes] - ref_obs_to_kp1(f["obs"][self.row[lanes]]))) <= 6e-8

    def check(self, ctx, env, real: str, *, obs: np.ndarray | None, last: int = 0) -> None:
        torch.cuda.synchronize()
        f = fixture()
        words, st = env.rng_state(), env.get_state()
        bad = np.flatnonzero(np.any(words != self.after[last], axis=1))
        assert bad.size == 0, (ctx, "words after", bad[:8], [str(f["label"][j]) if j >= 0 else "seed" for j in self.row[bad[:8]]])
        cast = (lambda x: x) if real == "f64" else (lambda x: x.astype(np.float32).astype(np.float64))
        assert np.array_equal(st["q"], self.q if real == "f64" else _two_float(self.q)), (ctx, "q", np.flatnonzero(np.any(st["q"] != self.q, axis=1))[:8])
        assert np.array_equal(st["goal_q"], cast(self.goal_q)), (ctx, "goal_q")
        assert not st["dq"].any() and not st["prev_action"].any(), (ctx, "dq / prev_action")
        assert np.max(np.abs(st["goal_pose6"] - self.goal_pose6)) <= (F64_TOL if real == "f64" else F32_POSE_TOL), (ctx, "goal_pose6")
        stage = env.info()["stage_index"].cpu().numpy()
        assert np.all(stage == self.stage), (ctx, "stage", np.unique(stage))
        if obs is not None:
            assert np.max(np.abs(obs[:, :kcfg.OBS_DIM] - self.obs)) <= (6e-8 if real == "f64" else 2e-6), (ctx, "observation")
        if last == 0:            # the reference's own record of the fixture rows
            lanes = np.flatnonzero(self.row >= 0)
            rows = self.row[lanes]
            assert np.array_equal(words[lanes], f["words_after"][rows]), (ctx, "fixture words")
            assert np.array_equal(st["q"][lanes], f["initial_q"][rows] if real == "f64" else _two_float(f["initial_q"][rows])), (ctx, "fixture initial_q")
            assert np.array_equal(st["goal_q"][lanes], cast(f["goal_q"][rows])), (ctx, "fixture goal_q")
            assert np.max(np.abs(st["goal_pose6"][lanes] - f["goal_pose6"][rows])) <= (F64_TOL if real == "f64" else F32_POSE_TOL), (ctx, "fixture goal_pose6")
            if obs is not None:
                assert np.max(np.abs(obs[lanes, :kcfg.OBS_DIM] - ref_obs_to_kp1(f["obs"][rows]))) <= (6e-8 if real == "f64" else 2e-6), (ctx, "fixture obs")


@lru_cache(maxsize=None)
def _batch(group: str, stage: int, resets: int = 1) -> Batch:
    """computed once per case and shared; nothing modifies it"""
    return Batch(group, stage, resets)


def _make_env(group: str, stage: int, real: str, *, pitch: int | None = None, n: int = N):
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    env = ArmKinematicVecEnv(_env_config(group, ONE_STEP), n, seed=5, real=real)
    env.set_curriculum_stage(stage)
    if pitch is not None:
        env.set_obs_stride(pitch)
    return env


def _far_action(dtype, n: int = N) -> torch.Tensor:
    return torch.ones((n, 7), dtype=dtype, device=DEV)


def _all_done(done: torch.Tensor, ctx) -> None:
    assert bool((done & 3).ne(0).all()), (ctx, "an env did not finish its one-step episode")


# ============================================================================== 1. kp1_reset_kernel and the step kernel's auto-reset
@pytest.mark.parametrize("real", ["f64", "f32"])
@pytest.mark.parametrize("group,stage", CASES)
def test_reset_and_step_kernels(group, stage, real):
    b = _batch(group, stage)
    env = _make_env(group, stage, real)
    env.reset()
    env.set_rng_state(b.words)
    obs = env.reset().cpu().numpy()
    b.check((group, stage, real, "kp1_reset_kernel"), env, real, obs=obs)
    env.set_rng_state(b.words)
    obs, _, done = env.step(_far_action(env.dtype))
    _all_done(done, (group, stage, real))
    b.check((group, stage, real, "kp1_step_kernel"), env, real, obs=obs.cpu().numpy())
    env.close()


@pytest.mark.parametrize("real", ["f64", "f32"])
@pytest.mark.parametrize("group,stage", [("scene", 5), ("tiny_nodraw", 0), ("tiny_reverse", 0)])
def test_consecutive_resets_carry_the_buffered_half(group, stage, real):
    """three resets of every env, the second by the step kernel: the words after each are the restatement's, so each reset consumed exactly
    the halves numpy's does (tiny_nodraw stage 0: one half per reset, the 128-bit state moves on every second reset only)"""
    b = _batch(group, stage, 3)
    env = _make_env(group, stage, real)
    env.reset()
    env.set_rng_state(b.words)
    env.reset()
    assert np.array_equal(env.rng_state(), b.after[0])
    _, _, done = env.step(_far_action(env.dtype))
    _all_done(done, (group, stage, real))
    assert np.array_equal(env.rng_state(), b.after[1])
    obs = env.reset().cpu().numpy()
    b.check((group, stage, real, "third reset"), env, real, obs=obs, last=2)
    if group == "tiny_nodraw":
        moved = [np.any(b.after[r][:, :2] != (b.words if r == 0 else b.after[r - 1])[:, :2], axis=1) for r in range(3)]
        assert np.all(moved[0] != moved[1]) and np.all(moved[1] != moved[2])
    env.close()


# ============================================================================== 2. the trace
@pytest.mark.parametrize("real", ["f64", "f32"])
def test_route_stride_trace(real, monkeypatch):
    """test_step_trace_gpu's assertions (n = 1) on the scene trace: episodes of at most three steps, nine auto-resets inside step launches"""
    import conftest
    import test_env_parity_gpu as tp

    name = "route_stride_scene_s2_seed11"
    g = np.load(GOLDEN / f"trace_{name}.npz")
    assert len(g["reset_at_step"]) >= 9 and json.loads(str(g["meta"]))["stage"] == 2
    cfg = group_cfg_dict("scene", {"env.episode_length": 3, "env.termination.max_episode_steps": 3})
    monkeypatch.setitem(TRACES, name, SCENE)
    monkeypatch.setattr(tp, "load_golden_config", lambda cfg_name: kcfg.to_env_config(cfg, handoff_base_dirs=(GOLDEN,)) if cfg_name == SCENE
                        else conftest.load_golden_config(cfg_name))
    tp.test_step_trace_gpu(name, real)


# ============================================================================== 3. kp1_set_stage and per-replica stages
def _expected(cfg: kcfg.EnvConfig, words: np.ndarray, stages) -> dict:
    """the restatement's reset of every env from `words` at its own stage: the pair, the stride and the words after"""
    import route_stride_reset as rsr

    rr = cfg.route_reset
    settings = {"min_stride_by_stage": rr.min_stride_by_stage, "max_stride_by_stage": rr.max_stride_by_stage, "start_q_noise": rr.start_q_noise,
                "goal_q_noise": rr.goal_q_noise, "reverse_probability": rr.reverse_probability}
    route, lower, upper = np.array(rr.route_q), np.array(cfg.c.joints.lower[:]), np.array(cfg.c.joints.upper[:])
    n = len(words)
    out = {"q": np.zeros((n, 7)), "goal_q": np.zeros((n, 7)), "stride": np.zeros(n, dtype=np.int64), "words": np.zeros((n, 6), dtype=np.uint64)}
    for i in range(n):
        bg = rf.bitgen_of(words[i])
        out["q"][i], out["goal_q"][i], start, goal = rsr.sample(np.random.Generator(bg), route, settings, int(stages[i]), lower, upper)
        out["stride"][i], out["words"][i] = abs(goal - start), rf.words_of(bg)
    return out


def _assert_sampled(ctx, env, want: dict) -> None:
    """an f32 handle holds the expected pairs, bit for bit"""
    torch.cuda.synchronize()
    st = env.get_state()
    assert np.array_equal(env.rng_state(), want["words"]), (ctx, "words")
    assert np.array_equal(st["q"], _two_float(want["q"])), (ctx, "q")
    assert np.array_equal(st["goal_q"], want["goal_q"].astype(np.float32).astype(np.float64)), (ctx, "goal_q")


def test_set_stage_changes_the_stride_range():
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    cfg = _env_config("scene", ONE_STEP)
    env = ArmKinematicVecEnv(cfg, N, seed=3, real="f32")
    for stage, (lo, hi) in ((0, (1, 1)), (4, (12, 18)), (1, (2, 3)), (5, (16, 28))):
        env.set_curriculum_stage(stage)
        for kernel in ("kp1_reset_kernel", "kp1_step_kernel"):
            want = _expected(cfg, env.rng_state(), [stage] * N)
            assert want["stride"].min() == lo and want["stride"].max() == hi, (stage, want["stride"].min(), want["stride"].max())
            if kernel == "kp1_reset_kernel":
                env.reset()
            else:
                _all_done(env.step(_far_action(torch.float32))[2], stage)
            _assert_sampled((stage, kernel), env, want)
            assert np.all(env.info()["stage_index"].cpu().numpy() == stage)
    env.close()


def test_population_replicas_sample_their_own_stride_range():
    """K = 2 replicas of 65 envs (the boundary inside a wave) on stages 1 and 5 of one table: each replica's auto-resets draw from its own
    stride range, and the population equals two single handles bit for bit"""
    from rl_brain_trainer_amd.curriculum import PointCurriculum, PointCurriculumPopulation
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    cfg = _env_config("scene", ONE_STEP)
    n, seeds, stages = 65, [7, 8], [1, 5]
    kw = {"success_rate_threshold": 1.0, "window_episodes": 16, "min_episodes_per_stage": 1 << 20, "max_stage_index": cfg.n_stages - 1}   # never promotes
    pop = ArmKinematicPopulationVecEnv(cfg, seeds, n)
    pcur = PointCurriculumPopulation(**kw, initial_stage_indices=stages)
    pcur.attach(pop)
    singles = [ArmKinematicVecEnv(cfg, n, seed=s) for s in seeds]
    curs = [PointCurriculum(**kw, initial_stage_index=st) for st in stages]
    for env, cur in zip(singles, curs):
        cur.attach(env)
    obs = pop.reset()
    for k, env in enumerate(singles):
        assert torch.equal(env.reset(), obs[pop.rows(k)]), k
    lane_stage = np.repeat(stages, n)
    for t in range(3):
        want = _expected(cfg, pop.rng_state(), lane_stage)
        s = want["stride"]
        assert (s[:n].min(), s[:n].max()) == (2, 3) and (s[n:].min(), s[n:].max()) == (16, 28), (t, s[:n].max(), s[n:].min())
        act = _far_action(torch.float32, 2 * n)
        pop.step(act)
        _all_done(pop.done, t)
        for k, env in enumerate(singles):
            env.step(act[pop.rows(k)].contiguous())
        _assert_sampled((t, "population"), pop, want)
        info = pop.info()
        for k, env in enumerate(singles):
            r = pop.rows(k)
            assert torch.equal(env.obs, pop.obs[r]) and torch.equal(env.done, pop.done[r]) and torch.equal(env.terminal_obs, pop.terminal_obs[r]), (t, k)
            for name, plane in env.info().items():
                assert torch.equal(plane, info[name][..., r]), (t, k, name)
        assert np.array_equal(pop.rng_state(), np.concatenate([e.rng_state() for e in singles])), t
        assert np.array_equal(info["stage_index"].cpu().numpy(), lane_stage)
    pcur.close()
    pop.close()
    for cur, env in zip(curs, singles):
        cur.close()
        env.close()


# ============================================================================== 4. the fused kernels at hidden 64
@pytest.mark.parametrize("group,stage", [("scene", 5), ("tiny_reverse", 0)])
def test_rollout_step_kernel(group, stage):
    """rollout_step_kernel (forward + env step + auto-reset in one launch) against forward, then kp1_step, from the same words: every output
    and every info plane equal, the words equal (test_rollout_step_layerwise_gpu's criterion) -- and the restatement's"""
    from test_rollout_step_layerwise_gpu import _mlp

    b = _batch(group, stage)
    env_a, env_b = _make_env(group, stage, "f32", pitch=64), _make_env(group, stage, "f32", pitch=64)
    mlp, _ = _mlp(64, 1, 256, seed=64)
    obs_a, obs_b = env_a.reset().clone(), env_b.reset().clone()
    assert torch.equal(obs_a, obs_b)
    env_a.set_rng_state(b.words)
    env_b.set_rng_state(b.words)
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=DEV)   # noqa: E731
    noise = torch.randn((N, 7), generator=torch.Generator(device=DEV).manual_seed(4), device=DEV)
    a = {"value": z(N), "action": z(N, 7), "log_prob": z(N), "next_obs": z(N, 64), "reward": z(N), "done": z(N, dt=torch.uint8), "terminal_obs": z(N, 64)}
    c = {k: torch.zeros_like(v) for k, v in a.items()}
    clipped = z(N, 7)
    mlp.forward_env_step(env_a, obs_a, noise=noise, **a)
    mlp.forward(obs_b, noise=noise, value=c["value"], action=c["action"], clipped=clipped, log_prob=c["log_prob"])
    env_b.step_into(clipped, c["next_obs"], c["reward"], c["done"], c["terminal_obs"], True)
    _all_done(a["done"], (group, stage))
    for k in a:
        assert torch.equal(a[k], c[k]), k
    ia, ib = env_a.info(), env_b.info()
    for k in ib:
        assert torch.equal(ia[k], ib[k]), k
    assert np.array_equal(env_a.rng_state(), env_b.rng_state())
    b.check((group, stage, "rollout_step_kernel"), env_a, "f32", obs=a["next_obs"].cpu().numpy())
    mlp.close()
    env_a.close()
    env_b.close()


@pytest.mark.parametrize("group,stage", [("scene", 5), ("tiny_reverse", 0)])
def test_rollout_run_kernel(group, stage):
    """rollout_run_kernel over a span of 2 one-step episodes (two resets of every env inside one launch) against two forward_env_step
    launches from the same words: every output buffer, every info plane and the words equal (test_rollout_run_gpu's criterion) -- and the
    words after the second reset are the restatement's, which they can only be if the first reset consumed what numpy's did"""
    from test_rollout_run_gpu import OUTPUTS, _buffers, _mlp, _noise

    b = _batch(group, stage, 2)
    got = []
    for form in ("run", "steps"):
        env = _make_env(group, stage, "f32", pitch=64)
        mlp = _mlp(64, 1, seed=64, max_batch=256)
        buf = _buffers(2, N, 64)
        noise = _noise(2, N, 5)
        buf["obs"][0].copy_(env.reset())
        env.set_rng_state(b.words)
        if form == "run":
            mlp.rollout_run(env, buf["obs"], noise=noise, value=buf["value"], action=buf["action"], log_prob=buf["log_prob"], reward=buf["reward"],
                            done=buf["done"], terminal_obs=buf["terminal_obs"], first_step=0, n_steps=2, trackers=None, steps_per_call=N)
        else:
            for t in range(2):
                mlp.forward_env_step(env, buf["obs"][t], noise=noise[t], value=buf["value"][t], action=buf["action"][t], log_prob=buf["log_prob"][t],
                                     next_obs=buf["obs"][t + 1], reward=buf["reward"][t], done=buf["done"][t], terminal_obs=buf["terminal_obs"][t])
        torch.cuda.synchronize()
        _all_done(buf["done"][0], (group, form, 0))
        _all_done(buf["done"][1], (group, form, 1))
        b.check((group, stage, form), env, "f32", obs=buf["obs"][2].cpu().numpy(), last=1)
        got.append((buf, {k: v.clone() for k, v in env.info().items()}, env.rng_state().copy()))
        mlp.close()
        env.close()
    (ba, ia, wa), (bb, ib, wb) = got
    for k in OUTPUTS:
        assert torch.equal(ba[k], bb[k]), k
    for k in ib:
        assert torch.equal(ia[k], ib[k]), ("info", k)
    assert np.array_equal(wa, wb)


# ============================================================================== 5. dock mode, a second table, switching off
def test_dock_mode_ignores_the_route():
    """a dock-mode handle with the route set resets and auto-resets exactly as one without it (sample_dock_reset does not read route_reset)"""
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    dock = json.loads((GOLDEN / "configs" / "dock_workspace_handoff_noop_ft_12env_raw.json").read_text())
    dock["env"]["termination"] = {**dock["env"].get("termination", {}), "max_episode_steps": 1, "terminate_on_success": False}
    dock["env"]["episode_length"] = 1
    plain = kcfg.to_env_config(dock, handoff_base_dirs=(GOLDEN,))
    routed = kcfg.to_env_config(dock, handoff_base_dirs=(GOLDEN,))
    routed.route_reset = _env_config("scene").route_reset
    assert plain.mode_name == "dock" and routed.route_reset.active and not plain.route_reset.active
    a, c = ArmKinematicVecEnv(plain, N, seed=9), ArmKinematicVecEnv(routed, N, seed=9)
    assert torch.equal(a.reset(), c.reset())
    for _ in range(2):
        a.step(_far_action(torch.float32))
        c.step(_far_action(torch.float32))
        assert torch.equal(a.obs, c.obs) and torch.equal(a.done, c.done)
    sa, sc = a.get_state(), c.get_state()
    assert all(np.array_equal(sa[k], sc[k]) for k in sa) and np.array_equal(a.rng_state(), c.rng_state())
    a.close()
    c.close()


def test_second_table_is_seen_by_a_captured_graph_and_zero_points_restore_the_mixer():
    """one captured kp1_step (one-step episodes: every env resamples) replayed three times: on the table the handle was created with, after a
    second kp1_set_route_stride_reset (another table, other stride lists) and after a call with zero points"""
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    cfg = _env_config("scene", ONE_STEP)
    first = cfg.clone()            # set_route_stride_reset replaces the block of the config the env holds
    env = ArmKinematicVecEnv(cfg, N, seed=21)
    env.set_curriculum_stage(2)
    act, obs, rew, tobs = _far_action(torch.float32), torch.zeros((N, 56), device=DEV), torch.zeros(N, device=DEV), torch.zeros((N, 56), device=DEV)
    done = torch.zeros(N, dtype=torch.uint8, device=DEV)
    env.reset()
    env.step_into(act, obs, rew, done, tobs, True)       # once eagerly, before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.use_current_stream()
        env.step_into(act, obs, rew, done, tobs, True)
    env.use_current_stream()
    torch.cuda.synchronize()
    want = _expected(cfg, env.rng_state(), [2] * N)
    g.replay()
    _assert_sampled("first table", env, want)
    # another table: the head of the first one, shifted by 0.1 rad on joint 3; stride lists of other lengths; no noise, never reversed
    second = np.array(cfg.route_reset.route_q)[:200].copy()
    second[:, 3] += 0.1
    other = cfg.clone()
    other.route_reset = kcfg.RouteResetConfig(enabled=True, route_q=tuple(map(tuple, second)), min_stride_by_stage=(5, 6, 7), max_stride_by_stage=(5, 6, 9, 11))
    env.set_route_stride_reset(other.route_reset)
    want = _expected(other, env.rng_state(), [2] * N)
    assert want["stride"].min() == 7 and want["stride"].max() == 9
    assert np.all(np.any(want["q"] != _expected(first, env.rng_state(), [2] * N)["q"], axis=1))      # no env would land on the same start by the first table
    g.replay()
    _assert_sampled("second table", env, want)
    # zero points: the stage mixer again, as a handle that never had a route
    env.set_route_stride_reset(None)
    twin = ArmKinematicVecEnv(copy_without_route(cfg), N, seed=21)
    twin.set_curriculum_stage(2)
    twin.reset()
    twin.set_rng_state(env.rng_state())
    g.replay()
    twin.step(act)
    torch.cuda.synchronize()
    sa, sb = env.get_state(), twin.get_state()
    assert all(np.array_equal(sa[k], sb[k]) for k in ("q", "goal_q", "goal_pose6")) and np.array_equal(env.rng_state(), twin.rng_state())
    assert not np.any(sa["q"]) and not np.any(sa["goal_q"])           # the scene config's stages are the zero pose without noise
    env.close()
    twin.close()


def copy_without_route(cfg: kcfg.EnvConfig) -> kcfg.EnvConfig:
    out = cfg.clone()
    out.route_reset = kcfg.RouteResetConfig()
    return out


def test_refusals():
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    env = ArmKinematicVecEnv(_env_config("tiny_nodraw"), 4, seed=1)
    three = tuple(tuple([0.01 * i] * 7) for i in range(3))

    def call(**kw):
        rr = kcfg.RouteResetConfig(enabled=True, route_q=three, **kw)
        env.set_route_stride_reset(rr)

    before = env.rng_state().copy()
    with pytest.raises(ValueError, match="stage 1 needs a stride of at least 3"):
        call(min_stride_by_stage=(1, 3))
    with pytest.raises(ValueError, match="1..16 entries"):
        call(max_stride_by_stage=(1,) * 17)
    with pytest.raises(ValueError, match="negative"):
        call(start_q_noise=(0.0,) * 6 + (-1.0,))
    with pytest.raises(ValueError, match="at least two q waypoints"):
        env.set_route_stride_reset(kcfg.RouteResetConfig(enabled=True, route_q=three[:1]))
    env.reset()                                             # the handle still samples from the table it was created with
    st = env.get_state()
    assert np.all(np.isin(np.round(st["q"][:, 0], 6), [0.0, 0.01, 0.02])) and not np.array_equal(env.rng_state(), before)
    env.close()


# ============================================================================== 6. the trainer
def test_train_cli_runs_the_scene_config(tmp_path):
    """train.py on the scene config, 2 x 64, 8 envs x 16 steps, 2 iterations: plain and with --seeds 1,2; the summary carries the curriculum
    stage, and each replica's checkpoint equals its single run's (test_approach_population_gpu's criterion)"""
    from rl_brain_trainer_amd import checkpoint, train

    cfg = json.loads((GOLDEN / "configs" / f"{SCENE}.json").read_text())
    cfg["env"]["route_reset"]["route_path"] = str(GOLDEN / "synthetic_route.json")
    cfg_path = tmp_path / "scene.yaml"
    cfg_path.write_text(json.dumps(cfg))
    common = ["--config", str(cfg_path), "--total-timesteps", "256", "--n-envs", "8", "--n-steps", "16", "--batch-size", "64", "--hidden", "64",
              "--log-every", "0"]
    pop_root = tmp_path / "pop"
    train.main(common + ["--run-id", "p", "--artifact-root", str(pop_root), "--seeds", "1,2"])
    for s in (1, 2):
        single_root = tmp_path / f"single_{s}"
        train.main(common + ["--run-id", f"s{s}", "--artifact-root", str(single_root), "--seed", str(s)])
        summary = json.loads((single_root / "training_summary.json").read_text())
        assert "curriculum" in json.dumps(summary) and "stage" in json.dumps(summary), sorted(summary)
        a_zip, b_zip = pop_root / f"seed_{s}" / "model_latest.zip", single_root / "model_latest.zip"
        a, b = checkpoint.load_policy_state_dict(a_zip), checkpoint.load_policy_state_dict(b_zip)
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), s
        oa, ob = checkpoint.load_optimizer_state_dict(a_zip), checkpoint.load_optimizer_state_dict(b_zip)
        for i, st in ob["state"].items():
            for name, v in st.items():
                assert torch.equal(oa["state"][i][name], v), (s, i, name)
