"""The fp32 route handle -- the one train_route and the route population run on -- against the reference's traces and the fp64 oracle.

Four pieces: the four reference route traces replayed on the fp32 handle; a lockstep batch of fp32 device envs against fp64 oracle envs
over every route config; padded observation rows (the PPO pitch) against an unpadded twin; long dense routes that need the raised LDS
limit of kp1_route_nearest_kernel.

Ties.  The fp32 handle computes the gated quantities (q / position / orientation error, action and dq norm) with a few 1e-7 of noise, so
a comparison against a threshold may come out differently than in fp64 when the fp64 value sits within a small delta of the threshold.
Such ties are detected on the reference side (fp64 oracle or trace) and classified:
- a *state* tie (route_ready inputs, the base env's near-goal / success gates) can change what happens next (streak, hand-over, base
  dwell counter in the observation), so it taints the env until its next reset (trace) or drops it from the comparison (batch);
- a *step* tie (the low-motion branch at 2x the pose thresholds, the >= comparisons of no_progress, the regression flag, the orientation
  hit flag) changes only that step's outputs, so it excuses only the quantities it feeds, on that step.
A conjunction is only ambiguous when some term is tied and every other term holds (_and_ambiguous).

Observed on the MI355X: every error 5x or more below its bound (the test docstrings give the worst values).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import route_oracle as ro
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import route_config as rcfg
from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv, RouteVecEnv
from route_lockstep import (ERR_TOL, OBS_TOL, RESET_OBS_TOL, OracleBatch, Ties, Worst, _and_ambiguous, _check_resets, _check_step, _policy)  # noqa: F401
from test_env_parity_gpu import _two_float
from test_route_env_gpu import _cfg_dict, _golden_words

pytestmark = pytest.mark.gpu

# the tolerances of the fp32 handle, the tie classes and the step check live in route_lockstep.py, next to the randomised-config cases
CONFIGS = [("seq_prefix120", "route_curriculum_prefix120_routeobs_sequence2", 120),
           ("seq_prefix170", "route_curriculum_prefix170_routeobs_sequence2", 170),   # BASELINE configs[4]
           ("seq_prefix20", "route_curriculum_prefix20_sequence2", 20),
           ("single_default", "route_curriculum_default", 20)]


@pytest.fixture(scope="module")
def route_q() -> np.ndarray:
    return rcfg.load_route_q(GOLDEN / "synthetic_route.json")


def _configs(cfg_name: str, max_index: int) -> tuple[kcfg.EnvConfig, rcfg.RouteConfig, rcfg.RouteConfig]:
    """(base env config, route config for the device, an independent copy for the oracle)"""
    cfgd = _cfg_dict(cfg_name)
    return kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=max_index), rcfg.route_config_from_dict(cfgd, max_route_index=max_index)


# ============================================================================== 1. the reference traces on the fp32 handle
@pytest.mark.parametrize("name,cfg_name,max_index", CONFIGS)
def test_route_env_replays_reference_trace_f32(route_q, name, cfg_name, max_index):
    """One fp32 device env replays the reference's recorded episode stream, next to the fp64 oracle stepped in lockstep (which replays it
    bit for bit and supplies dq for the tie test).  Reset draws (fp64 on both handles) bit exact at every reset; reset q = the two-float
    rounding of the reference q; every untainted step compared on every output.  Floors: >= 90 % of the steps compared, >= 1 compared
    waypoint hand-over per trace.
    Observed on the MI355X, worst over the four traces: no state tie (every step compared; 19-335 hand-overs per trace), up to 730 step
    ties; components 0-12 3.2e-6 (ee_orientation_progress), orientation_regression 2.5e-6, reward 5.7e-6, components 13-15 2.7e-7,
    observation 1.3e-7, terminal observation 1.2e-7, reset observation 1.2e-7, q_error_norm 5.3e-8, nearest distance 4.5e-8."""
    g = np.load(GOLDEN / f"route_trace_{name}.npz")
    base, rc, rc_o = _configs(cfg_name, max_index)
    seed = int(g["seed"])
    env = RouteVecEnv(base, rc, route_q, 1, seed=seed, real="f32", reward_components=True)
    assert env.dtype == torch.float32 and env.obs_dim == g["obs"].shape[1]
    ora = ro.OracleRouteEnv(base, rc_o, ro.Route(route_q))
    ties = Ties(base, rc)
    worst = Worst()
    T = int(np.sum(~np.isnan(g["reward"])))
    row = t = k = 0
    compared = handovers = state_ties = step_ties = 0
    obs = env.reset().cpu().numpy()[0]
    while t < T:
        ctx = (name, "reset", k)
        ora.reset(seed=seed if k == 0 else None)
        assert np.array_equal(ora.rng_words(), _golden_words(g["rng_after"][k])), ctx      # the oracle is still on the trace
        assert np.array_equal(env.rng_state()[0], _golden_words(g["rng_after"][k])), ctx
        info = env.info()
        assert int(info["route_reset_mode"][0]) == int(g["reset_mode"][k]) and int(info["start_route_index"][0]) == int(g["start_index"][k]), ctx
        assert int(info["route_index"][0]) == int(g["route_index"][row]), ctx
        assert np.array_equal(env.get_state()["q"][0], _two_float(ora.base_state()["q"])), ctx
        worst.check("reset_obs", obs - g["obs"][row], RESET_OBS_TOL, ctx)
        row += 1
        k += 1
        tainted = done = False
        while not done and t < T:
            ctx = (name, "row", row)
            a64 = g["action"][row]
            o, r, d = env.step(torch.tensor(a64[None], dtype=torch.float32, device="cuda"))
            _, out = ora.step(a64)
            comps_ref = g["components"][row]
            assert np.max(np.abs(np.array(out.components[:]) - comps_ref)) <= 1e-12, ctx   # lockstep oracle = trace
            tie = ties.of(comps_ref[None], a64[None], ora.base_state()["dq"][None], np.array(out.error_growth[:])[None])
            tie = {key: bool(v[0]) for key, v in tie.items()}
            tainted = tainted or tie["state"]
            state_ties += int(tie["state"])
            step_ties += int(tie["low_motion"] or tie["no_progress"] or tie["regression"] or tie["ori_hit"])
            d = int(d[0])
            done = bool(d & 3)
            info = env.info()
            _, comps = env.reward_components()
            if not tainted:
                compared += 1
                gold_done = int(g["terminated"][row]) | (int(g["truncated"][row]) << 1) | (int(g["success"][row]) << 2)
                assert (d & 7) == gold_done, (ctx, d, gold_done)
                assert int(info["route_ready"][0]) == int(g["ready"][row]) and int(info["route_waypoint_success"][0]) == int(g["waypoint_success"][row]), ctx
                if not tie["regression"]:
                    assert int(info["route_regression"][0]) == int(out.route_regression), ctx
                if not tie["ori_hit"]:
                    assert int(info["route_orientation_hit"][0]) == int(out.orientation_hit), ctx
                _check_step(worst, ctx, tie, comps[:, 0].cpu().numpy().astype(np.float64), comps_ref, float(r[0]), g["reward"][row],
                            float(info["route_q_error_norm"][0]), g["q_error"][row], float(info["nearest_route_q_distance"][0]), g["nearest"][row])
                handovers += int(g["waypoint_success"][row])
                if done:
                    worst.check("terminal_obs", env.terminal_obs.cpu().numpy()[0] - g["obs"][row], OBS_TOL, ctx)
                else:
                    assert int(info["route_index"][0]) == int(g["route_index"][row]) and int(info["route_ready_streak"][0]) == int(g["streak"][row]), ctx
                    assert int(info["route_completed_waypoints"][0]) == int(g["completed"][row]), ctx
                    worst.check("obs", o.cpu().numpy()[0] - g["obs"][row], OBS_TOL, ctx)
            if done:
                obs = o.cpu().numpy()[0]
            row += 1
            t += 1
    print(f"\n[{name}] steps {T} compared {compared} hand-overs {handovers} state ties {state_ties} step ties {step_ties} worst {worst}")
    assert compared >= 0.9 * T, (compared, T)
    assert handovers >= 1
    env.close()


# ============================================================================== 2. lockstep batch vs the fp64 oracle
@pytest.mark.parametrize("name,cfg_name,max_index", CONFIGS)
def test_route_env_f32_lockstep_batch_vs_oracle(route_q, name, cfg_name, max_index):
    """300 fp32 device envs (ragged: not a multiple of the nearest kernel's 32 envs per block nor of the step kernel's block) and 300
    fp64 oracle envs on the same actions, every env on every step, until every env has been auto-reset inside the launch at least once.
    Any discrete disagreement must coincide with a tie on the oracle's side; a state tie drops the env.  Floors: <= 5 % dropped,
    > 50 compared hand-overs, >= 90 % of the envs' first auto-resets compared; surviving envs end with equal RNG words.
    Observed on the MI355X, worst over the four configs (90-120 steps each): at most 1 of 300 envs dropped, 11k-16k compared hand-overs,
    all 300 first auto-resets compared, up to 174 step ties; components 0-12 3.9e-6 (ee_orientation_progress), reward 6.7e-6,
    components 13-15 3.2e-7, observation 1.8e-7, reset observation 1.8e-7, terminal observation 1.3e-7, q_error_norm 9.8e-8,
    nearest distance 5.8e-8."""
    base, rc, rc_o = _configs(cfg_name, max_index)
    N, seed = 300, 4242
    env = RouteVecEnv(base, rc, route_q, N, seed=seed, reward_components=True)
    assert env.dtype == torch.float32
    ob = OracleBatch(base, rc_o, route_q, N, seed)
    ties = Ties(base, rc)
    worst = Worst()
    obs = env.reset().cpu().numpy()
    _check_resets(env, ob, np.arange(N), obs, worst, (name, "reset"))
    dl = np.array(base.c.joints.delta_limit[:]) * base.c.env.action_delta_scale
    group = np.arange(N) % 10
    rng = np.random.default_rng(7)
    alive = np.ones(N, dtype=bool)
    resets = np.zeros(N, dtype=np.int64)
    handovers = compared_resets = ready_steps = low_motion_steps = step_ties = 0
    od = env.obs_dim
    for step in range(400):
        if np.all(resets >= 1):
            break
        ctx = (name, "step", step)
        (cur,) = ob.fields("current_route_index")
        a = _policy(rng, group, route_q[cur], ob.state("q"), dl)
        o, r, d = env.step(torch.tensor(a, device="cuda"))
        o_dev, r_dev, d_dev = o.cpu().numpy(), r.cpu().numpy().astype(np.float64), d.cpu().numpy().astype(np.int64)
        t_dev = env.terminal_obs.cpu().numpy()
        info = {k: v.cpu().numpy() for k, v in env.info().items() if k.startswith("route_") or k == "nearest_route_q_distance"}
        _, comps = env.reward_components()
        c_dev = comps.cpu().numpy().T.astype(np.float64)
        outs, o_ref = [], np.zeros((N, od), dtype=np.float32)
        for i, e in enumerate(ob.envs):
            o_ref[i], out = e.step(a[i].astype(np.float64))
            outs.append(out)
        dq = ob.state("dq")
        ref = {k: np.array([getattr(out, k) for out in outs]) for k in ("reward", "terminated", "truncated", "success", "route_ready", "ready_streak",
                                                                         "waypoint_success", "route_regression", "orientation_hit", "route_index",
                                                                         "completed_waypoints", "q_error_norm", "nearest_route_q_distance")}
        c_ref = np.array([out.components[:] for out in outs])
        tie = ties.of(c_ref, a.astype(np.float64), dq, np.array([out.error_growth[:] for out in outs]))
        alive &= ~tie["state"]
        step_ties += int(np.sum(alive & (tie["low_motion"] | tie["no_progress"] | tie["regression"] | tie["ori_hit"])))
        s = np.flatnonzero(alive)
        done_ref = (ref["terminated"] | ref["truncated"]).astype(bool)
        done_dev = (d_dev & 3) != 0
        ref_bits = ref["terminated"] | (ref["truncated"] << 1) | (ref["success"] << 2)
        bad = s[(d_dev[s] & 7) != ref_bits[s]]
        assert bad.size == 0, (ctx, "done bits", bad[:8], d_dev[bad[:8]], ref_bits[bad[:8]])
        for key_dev, key_ref in (("route_ready", "route_ready"), ("route_waypoint_success", "waypoint_success")):
            bad = s[info[key_dev][s].astype(np.int64) != ref[key_ref][s]]
            assert bad.size == 0, (ctx, key_dev, bad[:8])
        for key_dev, key_ref, tkey in (("route_regression", "route_regression", "regression"), ("route_orientation_hit", "orientation_hit", "ori_hit")):
            bad = s[(info[key_dev][s].astype(np.int64) != ref[key_ref][s]) & ~tie[tkey][s]]
            assert bad.size == 0, (ctx, key_dev, bad[:8])
        go = s[~done_ref[s]]   # the episode goes on: the wrapper's counters and the step's observation
        for key_dev, key_ref in (("route_index", "route_index"), ("route_ready_streak", "ready_streak"), ("route_completed_waypoints", "completed_waypoints")):
            bad = go[info[key_dev][go] != ref[key_ref][go]]
            assert bad.size == 0, (ctx, key_dev, bad[:8])
        worst.check("obs", o_dev[go] - o_ref[go], OBS_TOL, ctx)
        fin = s[done_ref[s]]
        worst.check("terminal_obs", t_dev[fin] - o_ref[fin], OBS_TOL, ctx)
        sub = {k: v[s] for k, v in tie.items()}
        _check_step(worst, ctx, sub, c_dev[s], c_ref[s], r_dev[s], ref["reward"][s], info["route_q_error_norm"][s].astype(np.float64),
                    ref["q_error_norm"][s], info["nearest_route_q_distance"][s].astype(np.float64), ref["nearest_route_q_distance"][s])
        handovers += int(ref["waypoint_success"][s].sum())
        ready_steps += int(ref["route_ready"][s].sum())
        low_motion_steps += int(np.sum((c_ref[s, 6] > 0) & (c_ref[s, 14] > float(rc.reward.route_ready_pos_threshold_m))))
        # auto-resets: the device reset inside the launch; reset the oracle envs that finished and compare the fresh episodes
        for i in np.flatnonzero(done_ref):
            ob.obs[i] = ob.envs[i].reset()
        compared_resets += int(np.sum(resets[fin] == 0))
        resets += done_dev
        _check_resets(env, ob, fin, o_dev, worst, ctx)
    dropped = int(N - alive.sum())
    print(f"\n[{name}] steps {step} dropped {dropped} compared hand-overs {handovers} first resets {compared_resets} ready steps {ready_steps} "
          f"low-motion steps above the ready radius {low_motion_steps} step ties {step_ties} worst {worst}")
    assert np.all(resets >= 1), int(np.sum(resets == 0))
    assert dropped <= N // 20, dropped
    assert handovers > 50 and compared_resets >= 0.9 * N and ready_steps > 0 and low_motion_steps > 0
    s = np.flatnonzero(alive)
    assert np.array_equal(env.rng_state()[s], np.stack([ob.envs[i].rng_words() for i in s]))
    env.close()


# ============================================================================== 3. padded observation rows
def _servo(env: RouteVecEnv, base: kcfg.EnvConfig, g: torch.Generator) -> torch.Tensor:
    """servo toward the current goal with noise, every 5th env uniform noise (computed from the device state)"""
    st = env.get_state()
    dl = torch.tensor(np.array(base.c.joints.delta_limit[:]) * base.c.env.action_delta_scale, device="cuda", dtype=torch.float32)
    goal = torch.tensor(st["goal_q"], device="cuda", dtype=torch.float32)
    q = torch.tensor(st["q"], device="cuda", dtype=torch.float32)
    a = (0.8 * (goal - q) / dl + 0.05 * torch.randn(q.shape, device="cuda", generator=g)).clamp(-1, 1)
    a[::5] = torch.rand((len(a[::5]), 7), device="cuda", generator=g) * 2 - 1
    return a


def _check_padded(padded: torch.Tensor, twin: torch.Tensor, od: int, ctx) -> None:
    assert torch.equal(padded[:, :od], twin), ctx
    assert torch.count_nonzero(padded[:, od:]).item() == 0, ctx    # NaN counts as nonzero


@pytest.mark.parametrize("cfg_name,max_index,stride", [("route_curriculum_prefix120_routeobs_sequence2", 120, 128),   # 80 floats in 128
                                                       ("route_curriculum_prefix20_sequence2", 20, 64)])              # 56 floats in 64
def test_route_env_padded_obs_rows_match_unpadded_twin(route_q, cfg_name, max_index, stride):
    """A route handle writing into PPO's padded rows (set_obs_stride) next to an unpadded twin of the same seed: columns [0, obs_dim) of
    obs and terminal_obs bit identical through steps, in-launch auto-resets and an explicit reset(options=...); the pad stays exactly 0."""
    base, rc, rc2 = _configs(cfg_name, max_index)
    N = 300
    padded = RouteVecEnv(base, rc, route_q, N, seed=99)
    twin = RouteVecEnv(base, rc2, route_q, N, seed=99)
    od = twin.obs_dim
    padded.set_obs_stride(stride)
    assert padded.obs.shape == (N, stride) and od < stride
    _check_padded(padded.reset(), twin.reset(), od, "reset")
    g = torch.Generator(device="cuda").manual_seed(5)
    dones = 0
    for t in range(64):
        a = _servo(twin, base, g)
        _, _, d = padded.step(a)
        _, _, d2 = twin.step(a)
        assert torch.equal(d, d2), t
        dones += int(((d & 3) != 0).sum())
        _check_padded(padded.obs, twin.obs, od, ("obs", t))
        _check_padded(padded.terminal_obs, twin.terminal_obs, od, ("terminal_obs", t))
    assert dones > N // 4
    opts = {"route_index": 9, "start_route_index": 7, "initial_q": route_q[np.full(N, 7)] + 0.001, "initial_dq": np.zeros((N, 7)),
            "initial_prev_action": np.zeros((N, 7))}
    _check_padded(padded.reset(options=opts), twin.reset(options=opts), od, "explicit reset")
    for t in range(4):
        a = _servo(twin, base, g)
        padded.step(a)
        twin.step(a)
        _check_padded(padded.obs, twin.obs, od, ("obs after explicit reset", t))
    padded.close()
    twin.close()


def test_route_population_padded_obs_rows_match_single_handles(route_q):
    """The buffer layout PPO uses for a route population: K = 2 replicas in one handle at stride 128; block k equals, bit for bit, an
    unpadded RouteVecEnv of seed seeds[k], and the pad stays 0."""
    cfg_name, max_index = "route_curriculum_prefix120_routeobs_sequence2", 120
    base, rc, _ = _configs(cfg_name, max_index)
    seeds, n = [11, 500], 150
    pop = RoutePopulationVecEnv(base, rc, route_q, seeds, n)
    twins = [RouteVecEnv(base, _configs(cfg_name, max_index)[1], route_q, n, seed=s) for s in seeds]
    od = pop.obs_dim
    pop.set_obs_stride(128)
    obs = pop.reset()
    for k, tw in enumerate(twins):
        _check_padded(obs[pop.rows(k)], tw.reset(), od, ("reset", k))
    g = torch.Generator(device="cuda").manual_seed(6)
    dones = 0
    for t in range(64):
        acts = [_servo(tw, base, g) for tw in twins]
        _, _, d = pop.step(torch.cat(acts))
        dones += int(((d & 3) != 0).sum())
        for k, tw in enumerate(twins):
            _, _, d2 = tw.step(acts[k])
            assert torch.equal(d[pop.rows(k)], d2), (t, k)
            _check_padded(pop.obs[pop.rows(k)], tw.obs, od, ("obs", t, k))
            _check_padded(pop.terminal_obs[pop.rows(k)], tw.terminal_obs, od, ("terminal_obs", t, k))
    assert dones > n // 2
    opts = {"route_index": 12, "start_route_index": 11, "initial_q": route_q[np.full(2 * n, 11)], "initial_dq": np.zeros((2 * n, 7)),
            "initial_prev_action": np.zeros((2 * n, 7))}
    obs = pop.reset(options=opts)
    for k, tw in enumerate(twins):
        o1 = {key: (v[:n] if isinstance(v, np.ndarray) else v) for key, v in opts.items()}
        _check_padded(obs[pop.rows(k)], tw.reset(options=o1), od, ("explicit reset", k))
    pop.close()
    for tw in twins:
        tw.close()


# ============================================================================== 4. long routes: the raised-LDS nearest kernel
def _dense_route(route_q: np.ndarray, W: int) -> np.ndarray:
    """the synthetic route interpolated linearly in joint space to W waypoints (same start and end)"""
    s = np.linspace(0.0, route_q.shape[0] - 1.0, W)
    return np.stack([np.interp(s, np.arange(route_q.shape[0]), route_q[:, k]) for k in range(7)], axis=1)


@pytest.mark.parametrize("real,W", [("f64", 1200), ("f64", 2340), ("f32", 2400), ("f32", 4681)])
def test_route_env_long_route_nearest_kernel(route_q, real, W):
    """Dense routes whose joint table exceeds the default 64 KB of LDS (up to the 128 KB cap: 2340 waypoints in fp64, 4681 in fp32), the
    window widened to W - 1: the device dataset equals the oracle's, and every env's nearest_route_q_distance equals the fp64 minimum over
    the route of ||route_q[w] - q|| (q from get_state) and the oracle's, on every step of a short lockstep run."""
    cfg_name = "route_curriculum_prefix120_routeobs_sequence2"
    rq = _dense_route(route_q, W)
    base, rc, rc_o = _configs(cfg_name, W - 1)
    N, seed = 100, 31
    env = RouteVecEnv(base, rc, rq, N, seed=seed, real=real)
    route = ro.Route(rq)
    assert np.max(np.abs(env.poses6 - route.poses6)) <= 1e-12
    assert np.max(np.abs(env.route_progress_m - route.progress)) <= 1e-11
    assert np.array_equal(env.next_q_delta, route.next_q_delta) and np.array_equal(env.chunk_id, route.chunk_id)
    oracles = [ro.OracleRouteEnv(base, rc_o, route) for _ in range(N)]
    env.set_route_window(max_route_index=W - 1)     # the config's own window stops at 120
    env.reset()
    for i, o in enumerate(oracles):
        o.set_route_window(max_route_index=W - 1)
        o.reset(seed=seed + i)
    cur = np.array([o.field("current_route_index") for o in oracles])
    assert np.array_equal(env.info()["route_index"].cpu().numpy(), cur) and cur.max() > W // 2   # resets reach deep into the route
    tol = 1e-12 if real == "f64" else ERR_TOL
    dl = np.array(base.c.joints.delta_limit[:]) * base.c.env.action_delta_scale
    rng = np.random.default_rng(3)
    worst, dones = 0.0, 0
    for t in range(6):
        goal = rq[np.array([o.field("current_route_index") for o in oracles])]
        q = np.stack([o.base_state()["q"] for o in oracles])
        a = _policy(rng, np.arange(N) % 10, goal, q, dl)
        _, _, d = env.step(torch.tensor(a, device="cuda"))
        done = (d.cpu().numpy() & 3) != 0
        near_dev = env.info()["nearest_route_q_distance"].cpu().numpy().astype(np.float64)
        outs = [o.step(a[i].astype(np.float64))[1] for i, o in enumerate(oracles)]
        assert np.array_equal(done, np.array([out.terminated or out.truncated for out in outs], dtype=bool)), t
        # the distance belongs to the q the step reached; an env that finished is already reset, so its q is taken from the oracle
        q = np.where(done[:, None], np.stack([o.base_state()["q"] for o in oracles]), env.get_state()["q"])
        near_np = np.sqrt(np.min(np.sum((rq[None, :, :] - q[:, None, :]) ** 2, axis=2), axis=1))
        near_ref = np.array([out.nearest_route_q_distance for out in outs])
        worst = max(worst, float(np.max(np.abs(near_dev - near_np))), float(np.max(np.abs(near_dev - near_ref))))
        assert np.max(np.abs(near_dev - near_np)) <= tol, (t, np.max(np.abs(near_dev - near_np)))
        assert np.max(np.abs(near_dev - near_ref)) <= tol, (t, np.max(np.abs(near_dev - near_ref)))
        dones += int(done.sum())
        for i in np.flatnonzero(done):
            oracles[i].reset()
    print(f"\n[{real} W={W}] nearest worst {worst:.3g}, {dones} auto-resets")
    env.close()


@pytest.mark.parametrize("real,W", [("f64", 2341), ("f32", 4682)])
def test_route_env_refuses_route_over_lds_budget(route_q, real, W):
    """One waypoint past the 128 KB joint-table cap is refused at creation (host check, KP1_ERR_INVALID; nothing is launched)."""
    base, rc, _ = _configs("route_curriculum_prefix120_routeobs_sequence2", 120)
    with pytest.raises(ValueError, match="route too long"):   # native.check raises ValueError for KP1_ERR_INVALID and only for it
        RouteVecEnv(base, rc, _dense_route(route_q, W), 4, real=real)
