"""Lockstep parity of the route env against the fp64 oracle under randomised route configs: cases, reference pass, tie classification,
bounds, comparator.  Helper, not a test module.

tests/test_route_lockstep_cpu.py checks this side where there is no device; tests/test_route_lockstep_gpu.py feeds the comparator the
arrays of the f64 and the f32 handle; tests/test_route_env_f32_gpu.py uses the tie classes and the step check on the four shipped configs.

Cases.  tests/golden/route_config_fuzz.npz (make_golden_route_config_fuzz.py): override dicts on top of
route_curriculum_prefix120_routeobs_sequence2 -- random weights / thresholds / sequence / dwell / termination settings, directed cases for
each clause of route_ready, windows at the end of the route, one route with a repeated waypoint.

Reference pass.  N = 200 oracle envs (three waves + 8 lanes) are stepped for max_episode_steps + 8 steps on float32 actions computed from
the ORACLE's state only; a finished env is reset on its own, so the step's own (terminal) observation and the fresh episode's are both kept.

Noise of the fp32 handle (q is stored as a two-float pair and the kinematic chain is fp64; q, poses and all route arithmetic are fp32):
- q error ||goal - q|| over 7 joints, both operands rounded to fp32 (|q| < 4: half an ulp <= 2.4e-7 as test_route_env_f32_gpu.py
  counts it): <= sqrt(7) * 2 * 2.4e-7 = N_Q = 1.3e-6; a difference of two q errors 2 * N_Q.  The nearest-waypoint distance and the
  projection of curr_q - prev_q on the unit tangent are the same kind of quantity: N_Q.
- position error from fp32 poses (|x| < 1.5 m): N_POS = 1e-7, the term test_route_env_f32_gpu.py counted (coordinates below 1 m
  round by half an ulp 3e-8 per axis and operand: sqrt(3) * 6e-8); a difference of two 2 * N_POS.
- orientation error from fp32 angles (|a| < 4: half an ulp 2^-23 per operand): sqrt(3) * 2.4e-7 = N_ORI = 4.2e-7 (~5e-7); a difference of
  two 1e-6.
- action norm: the actions are bit identical; an fp32 sum of 7 squares and a sqrt: 4 * 2^-24 relative.  dq norm: one rounding of dq per
  joint (|dq| < 0.125: 3.7e-9) -> 8 * 2^-24 relative + 2e-8.
- the action smoothness penalty reads a^2 / 7 and (a - prev_a)^2 / 7: 8 * 2^-24 relative each; on the first step of an episode
  prev_action is a reset's fp64 draw that the handle keeps in fp32, which adds 2e-7 to the second (on no later step: prev_action is then the
  previous float32 action, bit identical).
Bound of weighted component k: |dev - ref| <= |w_k| * n_k + 16 * 2^-24 * |ref| + 1e-7 (component_bounds).  Component 6 divides the two
norms by their thresholds, so its n_k carries 1 / threshold.  The reward is compared as reward - sum(excused components) within the sum
of the bounds of the other summed components.  The observation: route_q_error = clip((goal - q) / delta_limit_j) carries two fp32 roundings of q
(2 * 2^-23 = 2.4e-7) over delta_limit_j (3e-6 on joint 0), every other entry 2e-6 (RESET_OBS_TOL: output rounding of normalised values), plus 4 * 2^-24 * |ref| + 1e-7.
At the four shipped configs every bound is below the constants test_route_env_f32_gpu.py used before (asserted in the CPU test).

Ties, classified on the reference side only (a conjunction is ambiguous iff some term is tied and every other term holds):
- state tie: route_ready's five clauses, the base env's near-goal and success gates.  The dwell comparison streak >= dwell and a streak
  carried over a hand-over are integer consequences of ready, so nothing else can turn a tie into a different state.  Taints the env until
  its next reset, where it is re-admitted if the device finished the episode on the same step with equal RNG words.
- step tie: low-motion branch (component 6), no-progress (component 12), the regression and orientation-hit flags: excuses what it feeds.
The three error differences come from the oracle (RouteStepOut.error_growth), never from a component divided by its weight.
"""
from __future__ import annotations

import copy
import json
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from conftest import GOLDEN
from oracle import route_oracle as ro
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import route_config as rcfg
from test_env_parity_gpu import _two_float

N_ENVS = 200
SEED = 4242
EXTRA_STEPS = 8
U = 2.0 ** -24
BASE = "route_curriculum_prefix120_routeobs_sequence2"

DELTA_GATE = 2e-6    # a gated quantity this close to its threshold is a tie: >= 1.5x the worst q-error bound, 4x the orientation one
DELTA_DIFF = 4e-6    # curr - prev of two such errors (no_progress, regression): two independent roundings, 2 x DELTA_GATE
N_Q, N_POS, N_ORI, N_ORI_DIFF = 1.3e-6, 1e-7, 4.2e-7, 1e-6
# the constants of the shipped-config tests (test_route_env_f32_gpu.py keeps asserting them)
OBS_TOL = 2e-5       # route_q_error = (goal - q) / dl with dl = 0.024 on joint 1 (|q| up to pi): 2 * 2.4e-7 / 0.024 = 2e-5 worst case
RESET_OBS_TOL = 2e-6  # at a reset q is the two-float rounding of the fp64 draw and the route keys index the fp64 table: fp32 output rounding
ERR_TOL = 1e-5       # q_error_norm, nearest_route_q_distance, components 13-15: north_star's fp32 pose bar
COMP_TOL = 2e-5      # components 0-12: largest weight 8.5 (ee_orientation_progress) x (2 x 5e-7 orientation noise) = 8.5e-6, 2.3x margin
REWARD_TOL = 5e-5    # sum of 13 components, each within COMP_TOL but in practice one or two dominate: 2.5 x COMP_TOL
F64_TOL, F64_Q_TOL = 1e-9, 1e-12
CLAUSES = ("q", "pos", "ori", "action", "dq")


def _and_ambiguous(vals: np.ndarray, thrs: np.ndarray, delta: float) -> np.ndarray:
    """all(vals[j] <= thrs[j]) evaluated on fp32-noisy vals ([m, N]): can the two precisions disagree?  Yes iff some term lies within
    delta of its threshold and every other term holds."""
    vals = np.atleast_2d(vals)
    tied = np.abs(vals - thrs[:, None]) < delta
    holds = vals <= thrs[:, None]
    return tied.any(axis=0) & (holds | tied).all(axis=0)


class Ties:
    """The gates of one route config, evaluated on the reference side (fp64)."""

    def __init__(self, base: kcfg.EnvConfig, rc: rcfg.RouteConfig) -> None:
        w, br, bt = rc.reward, base.c.reward, base.c.termination
        self.ready_thr = np.array([w.route_ready_q_threshold, w.route_ready_pos_threshold_m, w.route_ready_ori_threshold_rad,
                                   w.route_ready_action_threshold, w.route_ready_dq_threshold])
        self.low_motion_thr = 2.0 * np.array([w.route_ready_pos_threshold_m, w.route_ready_ori_threshold_rad])
        self.ori_hit_thr = float(w.route_ready_ori_threshold_rad)
        # base env: near-goal (dwell counter -> observation) and success gates on (position, orientation)
        ori_gate = bool(br.use_orientation_gate)
        self.base_gates = [np.array([br.near_goal_pos_threshold_m, br.near_goal_ori_threshold_rad if ori_gate else np.inf]),
                           np.array([bt.success_pos_threshold_m, bt.success_ori_threshold_rad if bt.require_orientation else np.inf])]

    def of(self, comps: np.ndarray, action: np.ndarray, dq: np.ndarray, growth: np.ndarray) -> dict[str, np.ndarray]:
        """comps [N, 17] fp64 reference components, action / dq [N, 7] fp64, growth [N, 3] = curr - prev of (q, position, orientation)
        error from the oracle -> bool [N] per tie class"""
        q_err, pos, ori = comps[:, 13], comps[:, 14], comps[:, 15]
        act_n, dq_n = np.linalg.norm(action, axis=1), np.linalg.norm(dq, axis=1)
        ready = _and_ambiguous(np.stack([q_err, pos, ori, act_n, dq_n]), self.ready_thr, DELTA_GATE)
        base = np.zeros_like(ready)
        for thr in self.base_gates:
            base |= _and_ambiguous(np.stack([pos, ori]), thr, DELTA_GATE)
        return {"state": ready | base,
                "low_motion": _and_ambiguous(np.stack([pos, ori]), self.low_motion_thr, DELTA_GATE),
                "no_progress": _and_ambiguous(-growth.T, np.zeros(3), DELTA_DIFF),   # all(curr >= prev) = all(-(curr - prev) <= 0)
                "regression": np.abs(growth[:, 0]) < DELTA_DIFF,
                "ori_hit": np.abs(ori - self.ori_hit_thr) < DELTA_GATE}


class Worst:
    """worst |device - reference| and worst error / bound per quantity, for the docstrings, the profile and the failure messages"""

    def __init__(self) -> None:
        self.v: dict[str, float] = {}
        self.ratio: dict[str, float] = {}

    def check(self, key: str, diff, tol, ctx) -> None:
        diff = np.abs(np.asarray(diff, dtype=np.float64))
        d = float(np.max(diff)) if diff.size else 0.0
        self.v[key] = max(self.v.get(key, 0.0), d)
        if diff.size:
            tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), diff.shape)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(tol > 0.0, diff / tol, np.where(diff > 0.0, np.inf, 0.0))
            self.ratio[key] = max(self.ratio.get(key, 0.0), float(np.max(ratio)))
            if not np.all(diff <= tol):
                at = np.unravel_index(int(np.argmax(ratio)), diff.shape)
                raise Mismatch((ctx, key, at, float(diff[at]), float(tol[at])))

    def __repr__(self) -> str:
        return json.dumps({k: float(f"{v:.3g}") for k, v in sorted(self.v.items())})


class Mismatch(AssertionError):
    pass


def _check_step(worst: Worst, ctx, tie: dict, comps_dev: np.ndarray, comps_ref: np.ndarray, r_dev, r_ref, q_err_dev, q_err_ref, near_dev, near_ref,
                bounds: dict | None = None) -> None:
    """the continuous outputs of one untainted step (one env or a batch of envs as rows).  bounds = None: the constants of the shipped
    configs; else component_bounds(...) of the same rows."""
    comps_dev, comps_ref = np.atleast_2d(comps_dev), np.atleast_2d(comps_ref)
    b = bounds or {"err": ERR_TOL, "q_err": ERR_TOL, "nearest": ERR_TOL, "comps": np.full(comps_ref[:, :13].shape, COMP_TOL), "reward": None}
    worst.check("q_error_norm", np.asarray(q_err_dev) - q_err_ref, b["q_err"], ctx)
    worst.check("nearest_route_q_distance", np.asarray(near_dev) - near_ref, b["nearest"], ctx)
    if bounds is None:
        worst.check("components_13_15", comps_dev[:, 13:16] - comps_ref[:, 13:16], b["err"], ctx)
    else:   # one key per error, so that the record shows the position error against its own (smallest) noise term
        err = np.broadcast_to(np.asarray(b["err"], dtype=np.float64), comps_ref[:, 13:16].shape)
        for k in (13, 14, 15):
            worst.check(f"component_{k:02d}", comps_dev[:, k] - comps_ref[:, k], err[:, k - 13], (ctx, rcfg.COMPONENT_NAMES[k]))
    worst.check("component_16_route_ready", comps_dev[:, 16] - comps_ref[:, 16], 0.0, ctx)
    lm, npg = np.atleast_1d(tie["low_motion"]), np.atleast_1d(tie["no_progress"])
    for k in range(13):
        skip = lm if k == 6 else (npg if k == 12 else np.zeros_like(lm))
        worst.check(f"component_{k:02d}", (comps_dev[:, k] - comps_ref[:, k])[~skip], b["comps"][:, k][~skip], (ctx, rcfg.COMPONENT_NAMES[k]))
    r_dev, r_ref = np.atleast_1d(r_dev), np.atleast_1d(r_ref)
    if bounds is None:
        ok = ~(lm | npg)
        worst.check("reward", (r_dev - r_ref)[ok], REWARD_TOL, ctx)
    else:   # every step: the excused components leave both sums
        excused = np.zeros(comps_ref[:, :13].shape, dtype=bool)
        excused[:, 6], excused[:, 12] = lm, npg
        diff = (r_dev - np.sum(comps_dev[:, :13] * excused, axis=1)) - (r_ref - np.sum(comps_ref[:, :13] * excused, axis=1))
        worst.check("reward", diff, np.sum(b["comps"] * ~excused, axis=1) if b["reward"] is None else b["reward"], ctx)


def component_bounds(rc: rcfg.RouteConfig, comps: np.ndarray, action_norm: np.ndarray, dq_norm: np.ndarray, a2: np.ndarray, da2: np.ndarray,
                     q_err: np.ndarray, nearest: np.ndarray, fresh: np.ndarray) -> dict:
    """fp32 bounds of one batch of reference rows (module docstring): comps [n, 17], the rest [n]; fresh = the row is the first step of
    its episode"""
    w = rc.reward
    n = comps.shape[0]
    one = np.ones(n)
    n_act, n_dq = 4 * U * action_norm, 8 * U * dq_norm + 2e-8
    noise = np.stack([
        abs(w.q_goal_progress_weight) * 2 * N_Q * one,
        abs(w.ee_position_progress_weight) * 2 * N_POS * one,
        abs(w.ee_orientation_progress_weight) * N_ORI_DIFF * one,
        abs(w.route_tangent_progress_weight) * N_Q * one,
        0.0 * one,
        0.0 * one,
        abs(w.low_motion_near_waypoint_bonus) * 0.5 * (n_act / max(w.route_ready_action_threshold, 1e-9) + n_dq / max(w.route_ready_dq_threshold, 1e-9)),
        abs(w.orientation_regression_penalty_weight) * N_ORI_DIFF * one,
        abs(w.q_route_regression_penalty_weight) * 2 * N_Q * one,
        abs(w.off_route_penalty_weight) * N_Q * one,
        abs(w.action_magnitude_weight) * 8 * U * a2 / 7.0 + abs(w.action_delta_weight) * (8 * U * da2 / 7.0 + 2e-7 * fresh),
        abs(w.dq_penalty_weight) * n_dq,
        0.0 * one], axis=1)
    rel = lambda ref: 16 * U * np.abs(ref) + 1e-7
    return {"comps": noise + rel(comps[:, :13]),
            "err": np.stack([N_Q * one, N_POS * one, N_ORI * one], axis=1) + rel(comps[:, 13:16]),
            "q_err": N_Q + rel(q_err), "nearest": N_Q + rel(nearest), "reward": None}


def obs_bounds(base: kcfg.EnvConfig, obs_ref: np.ndarray) -> np.ndarray:
    """fp32 bound of observation rows [n, od] taken after a step"""
    od = obs_ref.shape[-1]
    absolute = np.full(od, RESET_OBS_TOL)
    if od == rcfg.ROUTE_OBS_DIM:
        o, wd = rcfg.ROUTE_OBS_LAYOUT["route_q_error"]
        absolute[o:o + wd] = np.maximum(2 * 2.0 ** -23 / np.array(base.c.joints.delta_limit[:]), RESET_OBS_TOL)
    return absolute + 4 * U * np.abs(obs_ref.astype(np.float64)) + 1e-7


def _ulp32(x: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


# ============================================================================== the shipped-config batch helpers
def _policy(rng: np.random.Generator, group: np.ndarray, goal: np.ndarray, q: np.ndarray, dl: np.ndarray) -> np.ndarray:
    """noisy servo toward the current waypoint (70 %), near-zero actions (20 %: ready, dwell and the low-motion bonus), uniform noise (10 %)"""
    n = q.shape[0]
    a = np.clip(0.8 * (goal - q) / dl + rng.normal(0, 0.03, (n, 7)), -1, 1)
    still = group >= 7
    a[still] = rng.normal(0, 0.01, (int(still.sum()), 7))
    noise = group == 9
    a[noise] = rng.uniform(-1, 1, (int(noise.sum()), 7))
    return a.astype(np.float32)


class OracleBatch:
    """N serial fp64 oracle envs with env i seeded seed + i, as the device handle seeds its streams; windows = one (min, max) per env"""

    def __init__(self, base, rc, route_q, n: int, seed: int, windows: list | None = None) -> None:
        route = ro.Route(route_q)
        self.envs = [ro.OracleRouteEnv(base, rc, route) for _ in range(n)]
        for e, win in zip(self.envs, windows or []):
            e.set_route_window(min_route_index=win[0], max_route_index=win[1])
        self.obs = np.stack([e.reset(seed=seed + i) for i, e in enumerate(self.envs)])

    def state(self, key: str) -> np.ndarray:
        return np.stack([e.base_state()[key] for e in self.envs])

    def fields(self, *names: str) -> list[np.ndarray]:
        return [np.array([e.field(nm) for e in self.envs]) for nm in names]

    def words(self) -> np.ndarray:
        return np.stack([e.rng_words() for e in self.envs])


def _check_resets(env, ob: OracleBatch, idx: np.ndarray, dev_obs: np.ndarray, worst: Worst, ctx) -> None:
    """device state right after a reset of envs idx (initial or inside the step launch) against the oracle after its reset"""
    if idx.size == 0:
        return
    info = env.info()
    cur, start, mode = ob.fields("current_route_index", "start_route_index", "reset_mode")
    for key, ref in (("route_index", cur), ("start_route_index", start), ("route_reset_mode", mode)):
        dev = info[key].cpu().numpy()[idx]
        assert np.array_equal(dev, ref[idx]), (ctx, key, idx[dev != ref[idx]][:8])
    assert np.all(info["route_ready_streak"].cpu().numpy()[idx] == 0) and np.all(info["route_completed_waypoints"].cpu().numpy()[idx] == 0), ctx
    words = env.rng_state()[idx]
    ref_words = np.stack([ob.envs[i].rng_words() for i in idx])
    assert np.array_equal(words, ref_words), (ctx, idx[np.any(words != ref_words, axis=1)][:8])
    assert np.array_equal(env.get_state()["q"][idx], _two_float(ob.state("q")[idx])), ctx
    worst.check("reset_obs", dev_obs[idx] - ob.obs[idx], RESET_OBS_TOL, ctx)


# ============================================================================== cases
@dataclass(frozen=True)
class Case:
    name: str
    index: int
    overrides: dict = field(hash=False, compare=False)
    repeated_waypoint: int = -1
    seed: int = 0
    obs_dim: int = 0


def _merge(base: dict, over: dict) -> dict:
    out = dict(base)
    for k, v in over.items():
        out[k] = _merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else copy.deepcopy(v)
    return out


@lru_cache(maxsize=1)
def fixture():
    return np.load(GOLDEN / "route_config_fuzz.npz")


@lru_cache(maxsize=1)
def all_cases() -> tuple[Case, ...]:
    cases = json.loads(str(fixture()["cases"]))
    return tuple(Case(c["name"], k, c["overrides"], int(c.get("repeated_waypoint", -1)), int(c["seed"]), int(c["obs_dim"])) for k, c in enumerate(cases))


def case_named(name: str) -> Case:
    return next(c for c in all_cases() if c.name == name)


def chunks(size: int = 6) -> list[tuple[Case, ...]]:
    cs = all_cases()
    return [cs[i:i + size] for i in range(0, len(cs), size)]


@lru_cache(maxsize=1)
def synthetic_route() -> np.ndarray:
    return rcfg.load_route_q(GOLDEN / "synthetic_route.json")


def shipped_dict(name: str = BASE) -> dict:
    return json.loads((GOLDEN / "configs" / f"{name}.json").read_text())


def config_dict(case: Case) -> dict:
    return _merge(shipped_dict(), case.overrides)


def route_of(case: Case) -> np.ndarray:
    rq = np.array(synthetic_route())
    if case.repeated_waypoint > 0:
        rq[case.repeated_waypoint] = rq[case.repeated_waypoint - 1]
    return rq


def build_configs(cfgd: dict, max_route_index: int | None = None) -> tuple[kcfg.EnvConfig, rcfg.RouteConfig]:
    return kcfg.to_env_config(copy.deepcopy(cfgd)), rcfg.route_config_from_dict(cfgd, max_route_index=max_route_index)


# ============================================================================== the reference pass
STEP_KEYS = ("reward", "terminated", "truncated", "success", "route_ready", "ready_streak", "waypoint_success", "route_regression", "orientation_hit",
             "route_index", "completed_waypoints", "q_error_norm", "nearest_route_q_distance", "action_norm", "dq_norm", "tangent_norm", "base_terminated",
             "base_success", "base_invalid")
# recorded next to them on every step: what the bounds, the counts and a replay need
EXTRA_KEYS = ("comps", "growth", "step_obs", "a2", "da2", "target", "last", "first", "fresh", "actions", "done")


@dataclass
class Reference:
    """One oracle pass.  The layout as_device, tests/test_route_lockstep_gpu.py::device_pass and compare share: every per-step array is
    [T, n, ...] and holds the step's own values; post / reset0 hold the state after the auto-reset / the initial reset."""
    cfgd: dict
    base: kcfg.EnvConfig
    rc: rcfg.RouteConfig
    route_q: np.ndarray
    n: int
    seed: int
    windows: list | None
    T: int
    seq: bool                   # sequence env (else the single-waypoint env)
    n_waypoints: int
    win_max: np.ndarray         # [n] the window's max_route_index of each env
    reset0: dict                # reset_state() after the initial reset
    post: dict                  # reset_state() after each step's auto-resets, [T, n, ...] per key
    ties: dict                  # Ties.of per step, bool [T, n] per class
    clause_holds: np.ndarray    # [5, T, n]: does each clause of route_ready hold on the reference's values
    # STEP_KEYS: RouteStepOut fields
    reward: np.ndarray
    terminated: np.ndarray
    truncated: np.ndarray
    success: np.ndarray
    route_ready: np.ndarray
    ready_streak: np.ndarray
    waypoint_success: np.ndarray
    route_regression: np.ndarray
    orientation_hit: np.ndarray
    route_index: np.ndarray
    completed_waypoints: np.ndarray
    q_error_norm: np.ndarray
    nearest_route_q_distance: np.ndarray
    action_norm: np.ndarray
    dq_norm: np.ndarray
    tangent_norm: np.ndarray
    base_terminated: np.ndarray
    base_success: np.ndarray
    base_invalid: np.ndarray
    # EXTRA_KEYS
    comps: np.ndarray           # [T, n, 17]
    growth: np.ndarray          # [T, n, 3] RouteStepOut.error_growth
    step_obs: np.ndarray        # [T, n, od] float32: the step's own (for a finished env: terminal) observation
    a2: np.ndarray              # |a|^2 and |a - prev_action|^2
    da2: np.ndarray
    target: np.ndarray          # current / last route index before the step, first target of the running episode
    last: np.ndarray
    first: np.ndarray
    fresh: np.ndarray           # the step is the first of its episode (prev_action is a reset's draw)
    actions: np.ndarray         # [T, n, 7] float32
    done: np.ndarray


def lockstep_policy(rng: np.random.Generator, goal: np.ndarray, q: np.ndarray, dl: np.ndarray) -> np.ndarray:
    """By env index modulo 10: servo toward the current waypoint with gains 0.8 / 0.8 / 0.6 / 0.6 / 0.4 / 0.4 / 0.25 and noise 0.03 (the
    gains spread the step at which the action and the dq clause let go), a strong servo with large noise (0.15: position ready, action
    not), near-zero actions, uniform noise."""
    n = q.shape[0]
    group = np.arange(n) % 10
    gain = np.array([0.8, 0.8, 0.6, 0.6, 0.4, 0.4, 0.25, 0.8, 0.0, 0.0])[group]
    sigma = np.array([0.03, 0.03, 0.03, 0.01, 0.03, 0.01, 0.01, 0.15, 0.01, 0.0])[group]
    a = np.clip(gain[:, None] * (goal - q) / dl + sigma[:, None] * rng.normal(0, 1, (n, 7)), -1, 1)
    noise = group == 9
    a[noise] = rng.uniform(-1, 1, (int(noise.sum()), 7))
    return a.astype(np.float32)


def reference_pass(cfgd: dict, route_q: np.ndarray, actions: np.ndarray | None = None, n: int = N_ENVS, seed: int = SEED, action_seed: int = 0,
                   windows: list | None = None, steps: int | None = None) -> Reference:
    """The oracle's pass over one config.  actions = None: lockstep_policy on the oracle's state; else the given [T, n, 7] schedule (a mutant
    config replaying the reference's actions).  Arrays are [T, n, ...]: the step's own values, then the state after the auto-reset."""
    base, rc = build_configs(cfgd)
    ob = OracleBatch(base, rc, route_q, n, seed, windows)
    T = steps or int(base.c.termination.max_episode_steps) + EXTRA_STEPS
    od = ob.envs[0].obs_dim
    dl = np.array(base.c.joints.delta_limit[:]) * base.c.env.action_delta_scale
    ties = Ties(base, rc)
    rng = np.random.default_rng(1000 + action_seed)

    def reset_state() -> dict:
        cur, start, last, mode = ob.fields("current_route_index", "start_route_index", "last_route_index", "reset_mode")
        return {"obs": ob.obs.copy(), "q": ob.state("q"), "route_index": cur, "start_route_index": start, "last_route_index": last, "reset_mode": mode,
                "rng": ob.words()}

    reset0 = reset_state()
    first = reset0["route_index"].copy()        # the first target of each env's running episode
    fresh = np.ones(n, dtype=bool)
    win_max = np.array([w[1] for w in windows]) if windows else np.full(n, int(rc.reset.max_route_index))
    rec = {k: [] for k in STEP_KEYS + EXTRA_KEYS + ("post", "ties")}
    for t in range(T):
        (cur, last) = ob.fields("current_route_index", "last_route_index")
        a = actions[t] if actions is not None else lockstep_policy(rng, route_q[cur], ob.state("q"), dl)
        a64 = a.astype(np.float64)
        prev_action = ob.state("prev_action")
        outs, o_ref = [], np.zeros((n, od), dtype=np.float32)
        for i, e in enumerate(ob.envs):
            o_ref[i], out = e.step(a64[i])
            outs.append(out)
        for k in STEP_KEYS:
            rec[k].append(np.array([getattr(out, k) for out in outs]))
        comps = np.array([out.components[:] for out in outs])
        growth = np.array([out.error_growth[:] for out in outs])
        rec["comps"].append(comps)
        rec["growth"].append(growth)
        rec["step_obs"].append(o_ref)
        rec["a2"].append(np.sum(a64 * a64, axis=1))
        rec["da2"].append(np.sum((a64 - prev_action) ** 2, axis=1))
        rec["target"].append(cur)
        rec["last"].append(last)
        rec["first"].append(first.copy())
        rec["fresh"].append(fresh)
        rec["actions"].append(a)
        rec["ties"].append(ties.of(comps, a64, ob.state("dq"), growth))
        done = (rec["terminated"][-1] | rec["truncated"][-1]).astype(bool)
        rec["done"].append(done)
        fresh = done
        for i in np.flatnonzero(done):
            ob.obs[i] = ob.envs[i].reset()
        post = reset_state()     # for an env that goes on: its state after the step (obs = the last reset's, unused)
        first = np.where(done, post["route_index"], first)
        rec["post"].append(post)
    arrays = {k: np.array(rec[k]) for k in STEP_KEYS + EXTRA_KEYS}
    comps = arrays["comps"]
    vals = np.stack([comps[..., 13], comps[..., 14], comps[..., 15], arrays["action_norm"], arrays["dq_norm"]])
    return Reference(cfgd=cfgd, base=base, rc=rc, route_q=route_q, n=n, seed=seed, windows=windows, T=T, seq=bool(rc.sequence_enabled),
                     n_waypoints=route_q.shape[0], win_max=win_max, reset0=reset0,
                     post={k: np.array([p[k] for p in rec["post"]]) for k in rec["post"][0]},
                     ties={k: np.array([tt[k] for tt in rec["ties"]]) for k in rec["ties"][0]},
                     clause_holds=vals <= ties.ready_thr[:, None, None], **arrays)


DEVICE_KEYS = ("obs", "terminal_obs", "reward", "bits", "comps", "route_ready", "waypoint_success", "route_regression", "orientation_hit", "route_index",
               "ready_streak", "completed_waypoints", "start_route_index", "last_route_index", "reset_mode", "q_error_norm", "nearest_route_q_distance",
               "rng", "q")


def as_device(R: Reference, f32: bool = True) -> tuple[dict, dict]:
    """the reference's own pass laid out as a device returns it (values after the in-launch auto-reset), rounded through float32"""
    r32 = (lambda x: x.astype(np.float32).astype(np.float64)) if f32 else (lambda x: x.astype(np.float64))
    done = R.done
    dev = {"obs": np.where(done[..., None], R.post["obs"], R.step_obs), "terminal_obs": R.step_obs.copy(), "reward": r32(R.reward),
           "bits": (R.terminated | (R.truncated << 1) | (R.success << 2)).astype(np.int64), "comps": r32(R.comps),
           "route_ready": R.route_ready.copy(), "waypoint_success": R.waypoint_success.copy(), "route_regression": R.route_regression.copy(),
           "orientation_hit": R.orientation_hit.copy(), "route_index": R.post["route_index"].copy(),
           "ready_streak": np.where(done, 0, R.ready_streak), "completed_waypoints": np.where(done, 0, R.completed_waypoints),
           "start_route_index": R.post["start_route_index"].copy(), "last_route_index": R.post["last_route_index"].copy(),
           "reset_mode": R.post["reset_mode"].copy(), "q_error_norm": r32(R.q_error_norm), "nearest_route_q_distance": r32(R.nearest_route_q_distance),
           "rng": R.post["rng"].copy(), "q": _two_float(R.post["q"]) if f32 else R.post["q"].copy()}
    reset0 = {k: v.copy() for k, v in R.reset0.items()}
    if f32:
        reset0["q"] = _two_float(reset0["q"])
    return reset0, dev


# ============================================================================== the comparator
COUNT_KEYS = ("ready_not_reached", "handover_carried", "handover_cleared", "sequence_success_at_route_end", "sequence_success_cut_by_window",
              "success_without_termination", "base_success_suppressed", "zero_tangent")


class Report:
    def __init__(self) -> None:
        self.worst = Worst()
        self.nonzero = np.zeros(13, dtype=np.int64)
        self.sole = {c: 0 for c in CLAUSES}
        self.counts = {k: 0 for k in COUNT_KEYS + ("env_steps", "compared_env_steps", "pairs", "excused_pairs", "state_tied_envs", "dropped_envs",
                                                   "first_resets", "compared_first_resets", "handovers")}

    def summary(self) -> dict:
        return {"counts": dict(self.counts), "sole_failing_clause": dict(self.sole), "nonzero": self.nonzero.tolist(),
                "worst_error": {k: float(f"{v:.3g}") for k, v in sorted(self.worst.v.items())},
                "worst_error_over_bound": {k: float(f"{v:.3g}") for k, v in sorted(self.worst.ratio.items())}}


def _exact(key: str, a: np.ndarray, b: np.ndarray, idx: np.ndarray, ctx) -> None:
    a, b = np.asarray(a)[idx], np.asarray(b)[idx]
    bad = (a != b) if a.ndim == 1 else np.any(a != b, axis=tuple(range(1, a.ndim)))
    if np.any(bad):
        raise Mismatch((ctx, key, idx[bad][:8].tolist(), a[bad][:4].tolist(), b[bad][:4].tolist()))


def _check_reset_state(R: Reference, worst: Worst, dev_state: dict, ref_state: dict, idx: np.ndarray, strict: bool, ctx) -> None:
    if idx.size == 0:
        return
    for key in ("route_index", "start_route_index", "last_route_index", "reset_mode", "rng"):
        if key == "last_route_index" and not R.seq:
            continue      # the single-waypoint env has no last index
        _exact(key, dev_state[key], ref_state[key], idx, ctx)
    q_ref = ref_state["q"][idx]
    if strict:
        worst.check("reset_q", dev_state["q"][idx] - q_ref, F64_Q_TOL, ctx)
        worst.check("reset_obs", dev_state["obs"][idx].astype(np.float64) - ref_state["obs"][idx], np.maximum(_ulp32(ref_state["obs"][idx]), F64_TOL), ctx)
    else:
        _exact("reset_q", dev_state["q"], _two_float(ref_state["q"]), idx, ctx)
        worst.check("reset_obs", dev_state["obs"][idx].astype(np.float64) - ref_state["obs"][idx], RESET_OBS_TOL, ctx)


def compare(R: Reference, reset0: dict, dev: dict, strict: bool = False, label: str = "") -> Report:
    """dev / reset0 as as_device lays them out.  strict = the f64 handle: nothing is a tie, every env-step is compared, counters / flags /
    indices / RNG words exact, reward and components within 1e-9, observations within one float32 ulp or 1e-9."""
    rep = Report()
    worst = rep.worst
    n, T = R.n, R.T
    od = R.step_obs.shape[-1]
    _check_reset_state(R, worst, reset0, R.reset0, np.arange(n), strict, (label, "reset"))
    tainted = np.zeros(n, dtype=bool)
    ever = np.zeros(n, dtype=bool)
    resets = np.zeros(n, dtype=np.int64)
    dwell = int(R.base.c.termination.success_dwell_steps)
    no_tie = np.zeros(n, dtype=bool)
    for t in range(T):
        ctx = (label, "step", t)
        tie = {k: (no_tie if strict else v[t]) for k, v in R.ties.items()}
        tainted |= tie["state"]
        ever |= tie["state"]
        s = np.flatnonzero(~tainted)
        done = R.done[t]
        ref_bits = R.terminated[t] | (R.truncated[t] << 1) | (R.success[t] << 2)
        _exact("done bits", dev["bits"][t] & 7, ref_bits, s, ctx)
        _exact("route_ready", dev["route_ready"][t], R.route_ready[t], s, ctx)
        _exact("route_waypoint_success", dev["waypoint_success"][t], R.waypoint_success[t], s, ctx)
        _exact("route_regression", dev["route_regression"][t], R.route_regression[t], s[~tie["regression"][s]], ctx)
        _exact("route_orientation_hit", dev["orientation_hit"][t], R.orientation_hit[t], s[~tie["ori_hit"][s]], ctx)
        go, fin = s[~done[s]], s[done[s]]
        for key in ("route_index", "ready_streak", "completed_waypoints", "last_route_index", "start_route_index", "reset_mode", "rng"):
            ref = R.post[key][t] if key in R.post else getattr(R, key)[t]
            if key == "last_route_index" and not R.seq:
                continue
            _exact(key, dev[key][t], ref, go, ctx)
        _exact("ready_streak after reset", dev["ready_streak"][t], np.zeros(n, dtype=np.int64), fin, ctx)
        _exact("completed_waypoints after reset", dev["completed_waypoints"][t], np.zeros(n, dtype=np.int64), fin, ctx)
        sub = {k: v[s] for k, v in tie.items()}
        if strict:
            tol = np.full((s.size, 13), F64_TOL)
            b = {"comps": tol, "err": F64_TOL, "q_err": F64_TOL, "nearest": F64_TOL, "reward": F64_TOL}
            step_tol = lambda ref: np.maximum(_ulp32(ref), F64_TOL)
        else:
            b = component_bounds(R.rc, R.comps[t][s], R.action_norm[t][s], R.dq_norm[t][s], R.a2[t][s], R.da2[t][s], R.q_error_norm[t][s],
                                 R.nearest_route_q_distance[t][s], R.fresh[t][s])
            step_tol = lambda ref: obs_bounds(R.base, ref)
        _check_step(worst, ctx, sub, dev["comps"][t][s], R.comps[t][s], dev["reward"][t][s], R.reward[t][s], dev["q_error_norm"][t][s], R.q_error_norm[t][s],
                    dev["nearest_route_q_distance"][t][s], R.nearest_route_q_distance[t][s], bounds=b)
        worst.check("obs", dev["obs"][t][go].astype(np.float64) - R.step_obs[t][go], step_tol(R.step_obs[t][go]), ctx)
        worst.check("terminal_obs", dev["terminal_obs"][t][fin].astype(np.float64) - R.step_obs[t][fin], step_tol(R.step_obs[t][fin]), ctx)
        if strict:
            worst.check("q", dev["q"][t][go] - R.post["q"][t][go], F64_Q_TOL, ctx)
        # the fresh episodes of the envs that finished
        dev_state = {k: dev[k][t] for k in ("obs", "q", "route_index", "start_route_index", "last_route_index", "reset_mode", "rng")}
        _check_reset_state(R, worst, dev_state, {k: v[t] for k, v in R.post.items()}, fin, strict, ctx)
        # a tainted env whose episode ended on both sides on this step with equal RNG words starts its next episode clean
        back = np.flatnonzero(tainted & done & ((dev["bits"][t] & 3) != 0) & np.all(dev["rng"][t] == R.post["rng"][t], axis=1))
        tainted[back] = False
        # ---- counts over the compared env-steps
        c = rep.counts
        c["env_steps"] += n
        c["compared_env_steps"] += int(s.size)
        c["pairs"] += int(s.size) * 13
        c["excused_pairs"] += int(sub["low_motion"].sum() + sub["no_progress"].sum())
        c["first_resets"] += int(np.sum(done & (resets == 0)))
        c["compared_first_resets"] += int(np.sum(resets[fin] == 0))
        resets += done
        excused = np.zeros((s.size, 13), dtype=bool)
        excused[:, 6], excused[:, 12] = sub["low_motion"], sub["no_progress"]
        rep.nonzero += np.sum((R.comps[t][s][:, :13] != 0.0) & ~excused, axis=0)
        holds = R.clause_holds[:, t][:, s]
        for j, name in enumerate(CLAUSES):
            rep.sole[name] += int(np.sum(~holds[j] & (holds.sum(axis=0) == 4)))
        ready, wps, succ, term = (x[t][s].astype(bool) for x in (R.route_ready, R.waypoint_success, R.success, R.terminated))
        handover = wps & ~succ & R.seq
        c["handovers"] += int(handover.sum())
        c["ready_not_reached"] += int(np.sum(ready & ~wps & (dwell > R.ready_streak[t][s])))
        c["handover_carried"] += int(np.sum(handover & (R.ready_streak[t][s] > 0)))
        c["handover_cleared"] += int(np.sum(handover & (R.ready_streak[t][s] == 0) & bool(R.rc.reset_ready_streak_on_advance)))
        seq_len = max(int(R.rc.sequence_length), 1)
        c["sequence_success_at_route_end"] += int(np.sum(succ & R.seq & (R.target[t][s] == R.n_waypoints - 1)))
        c["sequence_success_cut_by_window"] += int(np.sum(succ & R.seq & (R.last[t][s] == np.minimum(R.win_max[s], R.n_waypoints - 1)) &
                                                          (R.first[t][s] + seq_len - 1 > R.last[t][s])))
        c["success_without_termination"] += int(np.sum(succ & ~term & (not R.seq)))
        c["base_success_suppressed"] += int(np.sum((R.base_terminated[t][s] != 0) & (R.base_success[t][s] != 0) & (R.base_invalid[t][s] == 0) & ~succ & ~term &
                                                   (not R.seq)))
        c["zero_tangent"] += int(np.sum(R.tangent_norm[t][s] == 0.0))
    rep.counts["state_tied_envs"] = int(ever.sum())
    rep.counts["dropped_envs"] = int(tainted.sum())
    _exact("final rng", dev["rng"][T - 1], R.post["rng"][T - 1], np.flatnonzero(~tainted), (label, "end"))
    return rep


def check_case_caps(R: Reference, rep: Report) -> None:
    c = rep.counts
    assert c["state_tied_envs"] <= R.n // 20, c
    assert c["compared_first_resets"] >= 0.9 * c["first_resets"] and c["first_resets"] >= 0.9 * R.n, c
    assert c["excused_pairs"] < 0.02 * c["pairs"], c


class Totals:
    """the floors over all cases: every count over compared env-steps"""
    FLOORS = {**{k: 50 for k in ("ready_not_reached", "handover_carried", "handover_cleared")},
              **{k: 20 for k in ("sequence_success_at_route_end", "sequence_success_cut_by_window", "success_without_termination", "base_success_suppressed",
                                 "zero_tangent")}}

    def __init__(self) -> None:
        self.counts = {k: 0 for k in COUNT_KEYS}
        self.sole = {c: 0 for c in CLAUSES}
        self.cases_nonzero = np.zeros(13, dtype=np.int64)     # cases in which component k is non-zero on >= 50 compared, non-excused env-steps

    def add(self, rep: Report) -> None:
        for k in COUNT_KEYS:
            self.counts[k] += rep.counts[k]
        for c in CLAUSES:
            self.sole[c] += rep.sole[c]
        self.cases_nonzero += rep.nonzero >= 50

    def short(self) -> list:
        out = [(k, v) for k, v in self.counts.items() if v < self.FLOORS[k]]
        out += [("sole failing clause", c, v) for c, v in self.sole.items() if v < 50]
        out += [("component", rcfg.COMPONENT_NAMES[k], int(v)) for k, v in enumerate(self.cases_nonzero) if v < 5]
        return out
