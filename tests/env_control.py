"""The env handle's control surface against the fp64 oracle: oracle-side counterparts, the reset-option table, the comparison rules.
Helper, not a test module.

tests/test_env_control_cpu.py pins the oracle-side helpers where there is no device; tests/test_env_control_gpu.py drives an
``ArmKinematicVecEnv`` and an ``OracleVecEnv`` through the same calls and compares them with the rules below.

Oracle-side counterparts (on ``oracle.OracleVecEnv`` / ``OEnv``; kp1_oracle.c is not involved beyond its public functions):
``set_state`` (kp1_set_state), ``snapshot`` / ``restore`` (kp1_state_snapshot / kp1_state_restore), ``update_config`` (kp1_update_config),
``apply_dock_stage`` (what a bound dock curriculum tracker re-applies after every config upload), ``set_handoff``
(kp1_set_handoff_states), ``set_mode`` (kp1_set_mode: handle-wide) and ``reset`` (kp1_reset with options and a mask).

Option table.  All 32 subsets of the five array options of ``reset`` times ``policy_mode`` unset / the config's mode / the other mode: 96
named rows.  Which branch of ``reset_env`` (csrc/kp1_env_step.inc) a row reaches:
- ``q`` in the row: the given-start branch (initial_q clipped to the joint limits; rows 0, 5, 10, ... of the draw lie outside them); no
  sample is taken and I_STAGE is the handle's stage.  Without ``q``: ``sample_reset`` in the row's mode (``mode=other`` runs the other
  mode's sampler on this config) and I_STAGE is the sampled stage.
- ``dq`` / ``pa`` in the row: the given value (norms 0.1 .. 1, so the entry metrics are non-trivial); without them the sampler's value
  where it has one (dock hand-off states, the random-start pair sampler), else zeros.
- ``gp`` with ``gq``: both taken as given, goal_q NOT clipped (rows 1, 6, 11, ... lie outside the limits).  ``gp`` without ``gq``:
  goal_q = 0.  ``gq`` alone: clipped, goal pose = FK.  Neither, without ``q``: the sampled goal (its stored pose for a hand-off state, FK
  otherwise).  Neither, with ``q``: ``sample_reachable_target`` drawn from the env's stream AFTER the options were applied.
Rows 2, 6, 10, ... of the goal poses carry an orientation pi +- delta (delta >= 1e-3) away from the given start's, per axis, so the
orientation error wraps through +-pi on them (a delta that large is no tie at fp32: ulp(pi) = 2.4e-7).

Comparison rules: the constants of tests/test_env_parity_gpu.py, imported.  f64 handle: RNG words, counters and flags exact, state floats
within F64_TOL, observations within 6e-8, rewards within 1e-9, done bytes equal.  f32 handle, on state that is placed (by reset or set_state)
rather than stepped: q exactly ``_two_float(ref)``, dq / prev_action / goal_q exactly the fp32 cast, poses, error norms and entry metrics
within F32_POSE_TOL, observations within 2e-6, RNG words exact.  Pose angles are compared modulo 2 pi, as that module does.
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass

import numpy as np

from oracle import oracle as orc
from rl_brain_trainer_amd import config as kcfg
from test_env_parity_gpu import F32_POSE_TOL, F64_TOL, _thresholds, _two_float

N_ENVS = 130                       # three 64-lane workgroups, the last one holds two lanes
F64_OBS_TOL, F64_REWARD_TOL = 6e-8, 1e-9      # test_batched_parity_vs_oracle_f64
F32_PLACED_OBS_TOL = 2e-6          # test_reset_stream_gpu
F32_TIE = 2e-6                     # test_step_trace_gpu: a gated quantity this close to its threshold may decide differently at fp32

OPTION_KEYS = ("initial_q", "initial_dq", "initial_prev_action", "goal_q", "goal_pose6")
SHORT = {"initial_q": "q", "initial_dq": "dq", "initial_prev_action": "pa", "goal_q": "gq", "goal_pose6": "gp"}
STATE_KEYS = ("q", "dq", "prev_action", "goal_q", "goal_pose6")
OPTION_OF_STATE = dict(zip(STATE_KEYS, OPTION_KEYS))
ENTRY_FIELDS = ("entry_position_error_norm", "entry_orientation_error_norm", "entry_action_l2", "entry_dq_norm")
COUNTERS = (("step_count", "episode_step"), ("dwell_count", "dwell_count"), ("near_goal_entry_count", "near_goal_entry_count"),
            ("near_goal_drift_count", "near_goal_drift_count"))


# ============================================================================== option table
@dataclass(frozen=True)
class OptionRow:
    name: str
    keys: tuple
    mode: str | None      # the policy_mode option, None = not given


def other_mode(mode_name: str) -> str:
    return "dock" if mode_name == "approach" else "approach"


def option_table(config_mode: str) -> tuple:
    rows = []
    for bits in range(32):
        keys = tuple(k for j, k in enumerate(OPTION_KEYS) if (bits >> j) & 1)
        label = "+".join(SHORT[k] for k in keys) or "none"
        for tag, mode in (("unset", None), ("same", config_mode), ("other", other_mode(config_mode))):
            rows.append(OptionRow(f"{label}/mode={tag}", keys, mode))
    return tuple(rows)


def draw_options(cfg: kcfg.EnvConfig, n: int = N_ENVS, seed: int = 20261020) -> dict:
    """one seeded draw of [n, 7] / [n, 6] values for the five array options (module docstring)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(cfg.c.joints.lower[:]), np.array(cfg.c.joints.upper[:])
    span = hi - lo
    rows = np.arange(n)

    def joints(outside: np.ndarray) -> np.ndarray:
        q = rng.uniform(lo + 0.05 * span, hi - 0.05 * span, size=(n, 7))
        push = rng.uniform(0.05, 0.5, size=(n, 7)) * rng.choice([-1.0, 1.0], size=(n, 7))
        beyond = np.where(push > 0, hi + push, lo + push)
        sel = rng.random((n, 7)) < 0.4
        sel[:, 0] = True
        q[outside] = np.where(sel, beyond, q)[outside]
        return q

    def vectors() -> np.ndarray:
        d = rng.normal(size=(n, 7))
        return d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.1, 1.0, size=(n, 1))

    out = {"initial_q": joints(rows % 5 == 0), "goal_q": joints(rows % 5 == 1), "initial_dq": vectors(), "initial_prev_action": vectors()}
    pose = orc.fk_pose6(joints(np.zeros(n, bool)))
    start = orc.fk_pose6(np.clip(out["initial_q"], lo, hi))
    wrap = rows % 4 == 2
    delta = rng.uniform(1e-3, 0.2, size=(n, 3)) * rng.choice([-1.0, 1.0], size=(n, 3))
    pose[wrap, 3:] = (start[:, 3:] + rng.choice([-1.0, 1.0], size=(n, 3)) * (np.pi + delta))[wrap]
    out["goal_pose6"] = pose
    out["outside_initial_q"], out["outside_goal_q"], out["wrap_rows"] = rows % 5 == 0, rows % 5 == 1, wrap
    return out


def options_of(row: OptionRow, values: dict) -> dict:
    opts = {k: values[k] for k in row.keys}
    if row.mode is not None:
        opts["policy_mode"] = row.mode
    return opts


def reset_mask(n: int = N_ENVS) -> np.ndarray:
    """every third env plus the last one (of the two lanes of the last workgroup one is reset and one is not)"""
    mask = np.zeros(n, np.uint8)
    mask[1::3] = 1
    mask[-1] = 1
    return mask


# ============================================================================== oracle-side counterparts
def reset(ora: orc.OracleVecEnv, options: dict | None = None, mask: np.ndarray | None = None) -> np.ndarray:
    """kp1_reset(mask, options): option arrays are [n, w] or one row, like vec_env.reset"""
    arrays = {k: np.broadcast_to(np.asarray(options[k], np.float64), (ora.n, 6 if k == "goal_pose6" else 7))
              for k in OPTION_KEYS if options and options.get(k) is not None}
    mode = (options or {}).get("policy_mode")
    for i in range(ora.n):
        if mask is not None and not mask[i]:
            continue
        o = {k: v[i] for k, v in arrays.items()}
        if mode is not None:
            o["policy_mode"] = mode
        ora.reset_env(i, o or None)
    return ora.obs


def set_state(ora: orc.OracleVecEnv, *, q=None, dq=None, prev_action=None, goal_q=None, goal_pose6=None, capture_entry_metrics: bool = True) -> None:
    """kp1_set_state: the given fields as they are (no clipping), ee_pose6 = FK(q) when q is given, _capture_entry_metrics when asked"""
    given = {"q": q, "dq": dq, "prev_action": prev_action, "goal_q": goal_q, "goal_pose6": goal_pose6}
    given = {k: np.broadcast_to(np.asarray(v, np.float64), (ora.n, 6 if k == "goal_pose6" else 7)) for k, v in given.items() if v is not None}
    for i in range(ora.n):
        e = ora.envs[i]
        for k, v in given.items():
            getattr(e, k)[:] = [float(x) for x in v[i]]
        if "q" in given:
            ora.L.kp1o_fk_pose6(e.q, e.ee_pose6)
        if capture_entry_metrics:
            ora.L.kp1o_env_capture_entry_metrics(C.byref(e))


def snapshot(ora: orc.OracleVecEnv) -> bytes:
    return C.string_at(C.addressof(ora.envs), C.sizeof(ora.envs))


def restore(ora: orc.OracleVecEnv, snap: bytes) -> None:
    assert len(snap) == C.sizeof(ora.envs)
    C.memmove(ora.envs, snap, len(snap))


def update_config(ora: orc.OracleVecEnv, cfg: kcfg.EnvConfig) -> None:
    """kp1_update_config: the env scalars and the dock_reset block of ``cfg`` reach every env, nothing else does"""
    for i in range(ora.n):
        ora.envs[i].cfg.env = cfg.c.env
        ora.envs[i].cfg.dock_reset = cfg.c.dock_reset


def apply_dock_stage(ora: orc.OracleVecEnv, stage) -> None:
    """dock_apply_stage (csrc/kp1_dock_curriculum.inc) of one resolved stage record: what a bound dock curriculum tracker writes over the
    uploaded config when it is attached, at a promotion and after every later config upload.  Stages with a hand-off slice are not handled."""
    assert stage.handoff_count < 0
    for i in range(ora.n):
        c = ora.envs[i].cfg
        for key in ("action_delta_scale", "dock_residual_action_limit", "dock_delta_q_change_limit_scale"):
            setattr(c.env, key, float(getattr(stage, key)))
        for key in ("close_bucket_probability", "close_bucket_min_pos_error_m", "close_bucket_max_pos_error_m", "close_bucket_max_ori_error_rad",
                    "handoff_state_probability"):
            setattr(c.dock_reset, key, float(getattr(stage, key)))
        for key in ("close_init_q_noise", "init_q_noise"):
            getattr(c.dock_reset, key)[:] = list(getattr(stage, key)[:])


def set_handoff(ora: orc.OracleVecEnv, states: list) -> None:
    """kp1_set_handoff_states: every env draws its dock hand-off resets from ``states`` from now on (the array stays alive on ``ora``)"""
    holder = kcfg.EnvConfig(c=ora.cfg.c, handoff_states=list(states))
    ora._handoff = holder.handoff_array()
    for i in range(ora.n):
        ora.L.kp1o_env_set_handoff(C.byref(ora.envs[i]), C.cast(ora._handoff, C.c_void_p), len(states))


def observe(ora: orc.OracleVecEnv) -> np.ndarray:
    """kp1_observe: current_observation() of every env, [n, 56]"""
    out = np.zeros((ora.n, kcfg.OBS_DIM), np.float32)
    for i in range(ora.n):
        ora.L.kp1o_env_observe(C.byref(ora.envs[i]), out[i].ctypes.data_as(C.POINTER(C.c_float)))
    return out


def set_mode(ora: orc.OracleVecEnv, mode_name: str) -> None:
    """kp1_set_mode: one mode for all envs of the handle"""
    for i in range(ora.n):
        ora.envs[i].policy_mode = kcfg.MODE_NAMES[mode_name]


def transplant_state(src: orc.OracleVecEnv, dst: orc.OracleVecEnv) -> None:
    """the state bytes and the RNG of every env of ``src`` into ``dst``; config and hand-off buffer stay ``dst``'s own"""
    first, size = orc.OEnv.rng.offset, C.sizeof(orc.OEnv)
    for i in range(src.n):
        keep = (dst.envs[i].handoff, dst.envs[i].n_handoff)
        C.memmove(C.addressof(dst.envs[i]) + first, C.addressof(src.envs[i]) + first, size - first)
        dst.envs[i].handoff, dst.envs[i].n_handoff = keep


# ============================================================================== probes
def _wrap(d: np.ndarray) -> np.ndarray:
    return (d + np.pi) % (2 * np.pi) - np.pi


def pose_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    d = np.abs(a - b)
    d[..., 3:] = np.abs(_wrap(d[..., 3:]))
    return d


def oracle_arrays(ora: orc.OracleVecEnv) -> dict:
    names = ("q", "dq", "prev_action", "goal_q", "goal_pose6", "ee_pose6", "min_pos_error", *ENTRY_FIELDS, "episode_step", "dwell_count",
             "near_goal_entry_count", "near_goal_drift_count", "pre_near_goal_hit", "near_goal_hit", "last_reset_stage", "policy_mode")
    out = dict(zip(names, ora.fields(*names)))
    out["entry_metrics"] = np.stack([out[k] for k in ENTRY_FIELDS], axis=1)
    out["position_error_norm"] = np.linalg.norm(out["goal_pose6"][:, :3] - out["ee_pose6"][:, :3], axis=1)       # pose_utils.py:21-30
    out["orientation_error_norm"] = np.linalg.norm(_wrap(out["goal_pose6"][:, 3:] - out["ee_pose6"][:, 3:]), axis=1)
    out["rng"] = ora.rng_words()
    return out


def handle_arrays(env) -> dict:
    """every real, integer and RNG word a caller can read from the handle, as host arrays [n, ...] (fp64 where the handle is fp32)"""
    out = dict(env.get_state())
    info = env.info()
    for k in ("ee_pose6", "entry_metrics"):
        out[k] = info[k].double().cpu().numpy().T.copy()
    for k in ("position_error_norm", "orientation_error_norm", "min_position_error", "executed_delta_q_l2", "action_l2", "delta_q_change_l2"):
        out[k] = info[k].double().cpu().numpy().copy()
    for k in ("step_count", "dwell_count", "near_goal_entry_count", "near_goal_drift_count", "flags", "stage_index"):
        out[k] = info[k].cpu().numpy().copy()
    for k in ("q", "dq", "prev_action", "goal_q", "goal_pose6"):
        out["info_" + k] = info[k].double().cpu().numpy().T.copy()
    out["rng"] = env.rng_state()
    return out


def assert_same_words(a: dict, b: dict, rows=None, ctx: str = "") -> None:
    assert a.keys() == b.keys()
    for k in a:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert np.array_equal(x, y), f"{ctx}: {k} differs"


class Stats:
    """worst observed error per compared quantity, next to its bound"""

    def __init__(self) -> None:
        self.worst: dict = {}

    def within(self, name: str, err, bound: float, ctx: str = "") -> None:
        err = float(np.max(err)) if np.size(err) else 0.0
        self.worst[name] = [max(self.worst.get(name, [0.0])[0], err), bound]
        assert err <= bound, f"{ctx}: {name} off by {err:.3e} (bound {bound:.1e})"

    def report(self, test: str) -> None:
        print("ENV_CONTROL " + json.dumps({"test": test, "worst": self.worst}))


def _sel(a: np.ndarray, rows) -> np.ndarray:
    return a if rows is None else a[rows]


def compare_state(env, ora: orc.OracleVecEnv, real: str, stats: Stats, *, rows=None, ctx: str = "", stage: bool = True, norms: bool = True,
                  h: dict | None = None) -> dict:
    """the handle's state against the oracle's on ``rows`` (all envs by default), by the rules of the module docstring.  At f32 the rows'
    state must be placed, not stepped.  ``norms=False`` leaves the info view's error norms out: after a step they are the step's own, so
    for an env the step auto-reset they belong to the finished episode (the VecEnv's terminal info), not to the new state.  Returns the
    handle's arrays."""
    h = handle_arrays(env) if h is None else h
    o = oracle_arrays(ora)
    assert np.array_equal(_sel(h["rng"], rows), _sel(o["rng"], rows)), f"{ctx}: RNG words"
    for hk, ok in COUNTERS:
        assert np.array_equal(_sel(h[hk], rows), _sel(o[ok], rows)), f"{ctx}: {hk}"
    assert np.array_equal(_sel(h["flags"] & 3, rows), _sel(o["pre_near_goal_hit"] | (o["near_goal_hit"] << 1), rows)), f"{ctx}: flags"
    if stage:
        assert np.array_equal(_sel(h["stage_index"], rows), _sel(o["last_reset_stage"], rows)), f"{ctx}: stage index"
    inf_h, inf_o = np.isinf(_sel(h["min_position_error"], rows)), np.isinf(_sel(o["min_pos_error"], rows))
    assert np.array_equal(inf_h, inf_o), f"{ctx}: min_position_error"
    tol = F64_TOL if real == "f64" else F32_POSE_TOL
    if real == "f64":
        for k in ("q", "dq", "prev_action", "goal_q"):
            stats.within(f"f64 {k}", np.abs(_sel(h[k], rows) - _sel(o[k], rows)), F64_TOL, ctx)
    else:
        assert np.array_equal(_sel(h["q"], rows), _sel(_two_float(o["q"]), rows)), f"{ctx}: q is not the two-float pair of the reference"
        for k in ("dq", "prev_action", "goal_q"):
            assert np.array_equal(_sel(h[k], rows), _sel(o[k].astype(np.float32).astype(np.float64), rows)), f"{ctx}: {k} is not the fp32 cast"
    for k in ("goal_pose6", "ee_pose6"):
        stats.within(f"{real} {k}", pose_diff(_sel(h[k], rows), _sel(o[k], rows)), tol, ctx)
    stats.within(f"{real} entry_metrics", np.abs(_sel(h["entry_metrics"], rows) - _sel(o["entry_metrics"], rows)), tol, ctx)
    for k in ("position_error_norm", "orientation_error_norm") if norms else ():
        stats.within(f"{real} info {k}", np.abs(_sel(h[k], rows) - _sel(o[k], rows)), tol, ctx)
    fin = ~inf_h
    stats.within(f"{real} min_position_error", np.abs(_sel(h["min_position_error"], rows)[fin] - _sel(o["min_pos_error"], rows)[fin]), tol, ctx)
    for k in STATE_KEYS:      # the info views are the same fields (fp32 q: the high word of the pair)
        ref = h[k] if real == "f64" or k != "q" else h[k].astype(np.float32).astype(np.float64)
        assert np.array_equal(_sel(h["info_" + k], rows), _sel(ref, rows)), f"{ctx}: info view of {k} differs from get_state"
    return h


def compare_obs(obs_h: np.ndarray, obs_o: np.ndarray, real: str, stats: Stats, *, rows=None, ctx: str = "", name: str = "observation") -> None:
    """[n, 56 or 64] handle rows against [n, 56] oracle rows; the padding columns of a 64-float row are zero"""
    tol = F64_OBS_TOL if real == "f64" else F32_PLACED_OBS_TOL
    stats.within(f"{real} {name}", np.abs(_sel(obs_h[:, :kcfg.OBS_DIM], rows) - _sel(obs_o, rows)), tol, ctx)
    assert not np.any(obs_h[:, kcfg.OBS_DIM:]), f"{ctx}: padding columns of the observation rows are not zero"


# ============================================================================== lockstep runs
def draw_actions(arng: np.random.Generator, ora: orc.OracleVecEnv, cfg: kcfg.EnvConfig) -> np.ndarray:
    """test_batched_parity_vs_oracle_f64's mix: servo toward the goal for half the envs, uniform for the rest"""
    n = ora.n
    a = arng.uniform(-1.2, 1.2, size=(n, 7))
    goal_q, q = ora.fields("goal_q", "q")
    dl = np.array(cfg.c.joints.delta_limit[:]) * (cfg.c.env.dock_action_delta_scale or cfg.c.env.action_delta_scale)
    servo = 0.8 * (goal_q - q) / dl + arng.uniform(-0.01, 0.01, size=(n, 7))
    a[: n // 2] = servo[: n // 2]
    return a


def oracle_step(ora: orc.OracleVecEnv, a: np.ndarray, auto_reset: bool = True):
    """one oracle step with the finished envs reset one by one -> (obs after the reset, reward, done byte, kp1o_step_out records)"""
    out = ora.step_out(a)
    done = (out["terminated"] | (out["truncated"] << 1) | (out["success"] << 2) | (out["invalid"] << 3)).astype(np.uint8)
    if auto_reset:
        for i in np.nonzero(done & 3)[0]:
            ora.reset_env(int(i))
    return ora.obs, out["reward"], done, out


class Lockstep:
    """An env handle and an oracle stepped on the same actions.  f64: every step's done bytes, rewards, observations, counters, stage
    indices, joint positions and RNG words are compared.  f32: only what is exact there -- RNG words, step counts and stage indices -- on
    the envs that have met no tie (a gated error within F32_TIE of one of its thresholds) so far."""

    def __init__(self, env, ora: orc.OracleVecEnv, cfg: kcfg.EnvConfig, real: str, stats: Stats, seed: int = 1) -> None:
        import torch

        self.torch = torch
        self.env, self.ora, self.cfg, self.real, self.stats = env, ora, cfg, real, stats
        self.arng = np.random.default_rng(seed)
        self.tainted = np.zeros(ora.n, bool)
        self.pos_thr, self.ori_thr = _thresholds(cfg)
        self.t = 0
        self.resets = np.zeros(ora.n, np.int64)      # auto-resets per env since the last clear
        self.last_done = np.zeros(ora.n, np.uint8)

    def start(self, stage: int | None = None) -> None:
        if stage is not None:
            self.env.set_curriculum_stage(stage)
            self.ora.set_stage(stage)
        og = self.env.reset().cpu().numpy()
        oo = reset(self.ora)
        compare_obs(og, oo, self.real, self.stats, ctx="first reset", name="reset observation")
        assert np.array_equal(self.env.rng_state(), self.ora.rng_words())

    def step(self, *, auto_reset: bool = True, ctx: str = "") -> dict:
        torch, env, ora, real = self.torch, self.env, self.ora, self.real
        a = draw_actions(self.arng, ora, self.cfg)
        if real == "f32":
            a = a.astype(np.float32).astype(np.float64)
        og, rg, dg = env.step(torch.tensor(a, dtype=env.dtype, device=env.device), auto_reset=auto_reset)
        oo, ro, do, out = oracle_step(ora, a, auto_reset)
        ctx = f"{ctx} step {self.t}"
        self.t += 1
        if auto_reset:
            self.resets += (do & 3) != 0
        self.last_done = do
        info = env.info()
        h = {k: info[k].cpu().numpy() for k in ("step_count", "stage_index", "dwell_count", "near_goal_entry_count", "near_goal_drift_count")}
        o_step, o_stage, o_dwell, o_entry, o_drift, o_q = ora.fields("episode_step", "last_reset_stage", "dwell_count", "near_goal_entry_count",
                                                                     "near_goal_drift_count", "q")
        rng_h, rng_o = env.rng_state(), ora.rng_words()
        if real == "f64":
            dgn = dg.cpu().numpy()
            assert np.array_equal(dgn, do), f"{ctx}: done bytes differ at {np.nonzero(dgn != do)[0][:8]}"
            self.stats.within("f64 step reward", np.abs(rg.cpu().numpy() - ro), F64_REWARD_TOL, ctx)
            self.stats.within("f64 step observation", np.abs(og.cpu().numpy()[:, :kcfg.OBS_DIM] - oo), F64_OBS_TOL, ctx)
            self.stats.within("f64 step q", np.abs(info["q"].cpu().numpy().T - o_q), F64_TOL, ctx)
            for k, ref in (("step_count", o_step), ("stage_index", o_stage), ("dwell_count", o_dwell), ("near_goal_entry_count", o_entry),
                           ("near_goal_drift_count", o_drift)):
                assert np.array_equal(h[k], ref), f"{ctx}: {k}"
            assert np.array_equal(rng_h, rng_o), f"{ctx}: RNG words"
        else:
            tie = (np.min(np.abs(out["position_error_norm"][:, None] - self.pos_thr[None]), axis=1) < F32_TIE) | \
                  (np.min(np.abs(out["orientation_error_norm"][:, None] - self.ori_thr[None]), axis=1) < F32_TIE)
            self.tainted |= tie
            ok = ~self.tainted
            assert ok.sum() >= ora.n // 2, f"{ctx}: most envs met a tie, the run says nothing"
            assert np.array_equal(h["step_count"][ok], o_step[ok]), f"{ctx}: step counts"
            assert np.array_equal(h["stage_index"][ok], o_stage[ok]), f"{ctx}: stage indices"
            assert np.array_equal(rng_h[ok], rng_o[ok]), f"{ctx}: RNG words"
        return {"obs": og.clone(), "reward": rg.clone(), "done_handle": dg.clone(), "done": do, "stage_index": h["stage_index"].copy(),
                "step_count": h["step_count"].copy(), "out": out}

    def run(self, steps: int, **kw) -> None:
        for _ in range(steps):
            self.step(**kw)

    def run_until_all_reset(self, limit: int, ctx: str = "") -> list:
        """steps until every env has passed an auto-reset since now -> the per-step records"""
        self.resets[:] = 0
        recs = []
        while self.resets.min() == 0:
            assert len(recs) < limit, f"{ctx}: not every env reset within {limit} steps"
            recs.append(self.step(ctx=ctx))
        return recs
