"""Lockstep parity of the base env against the fp64 oracle: reference pass, tie classification, comparator.  Helper, not a test module.

tests/test_env_lockstep_cpu.py checks this side where there is no device; tests/test_env_lockstep_gpu.py feeds the comparator the
arrays of the f64 and the f32 handle.

Reference pass.  One case = (base config, reward block, stage).  N = 200 oracle envs (three full waves + 8 lanes) are stepped for
max_episode_steps + 8 steps on float32 actions computed from the ORACLE's state only; a finished env is reset on its own, so the last
observation of the old episode and the first of the new one are both kept.  The pass is laid out as the device returns it (values after
the in-launch auto-reset) next to the pre-reset values the tie classification and the bounds need.

Noise of the fp32 handle (what the tie widths and the bounds are derived from).  The handle carries q as a two-float pair (48 bits) and
runs the kinematic chain in fp64; pose6 and the goal pose are rounded to fp32 ONCE, everything after that is fp32.
- position: |x| < 2 m -> half an ulp = 2^-24 = 6.0e-8 per axis and operand; the error vector goal - curr carries two roundings per
  axis, its norm at most sqrt(3) * 1.2e-7 = 2.07e-7, plus ~3 * 2^-24 relative for the fp32 subtraction / square / sqrt:
  EPS_POS = 2.1e-7 + 3 * 2^-24 * value.
- orientation: |angle| < 4 -> half an ulp = 2^-23 = 1.19e-7, two roundings per axis, norm at most sqrt(3) * 2.4e-7 = 4.1e-7, plus the
  relative part of the wrap / norm arithmetic: EPS_ORI = 4.2e-7 + 3 * 2^-24 * value (4.8e-7 at the largest gate of these cases, 0.6 rad;
  the issue's "about 5e-7").
- DELTA_GATE = 2e-6 >= 3 * 4.8e-7 = 1.45e-6 (orientation), 9x the position noise.
- a difference of two SUCCESSIVE errors (drift counter, same_step_alignment_bonus, tiny_correction_bonus): the two current poses are rounded
  independently (2 * sqrt(3) * 6e-8 = 2.07e-7) and the shared goal rounding enters through the change of direction of the error vector,
  at most 2 * sqrt(3) * 6e-8 more: 4.2e-7 for position, 8.3e-7 for orientation in the worst case.  Three times that is 1.25e-6 and
  2.5e-6, so the 1e-6 of test_step_trace_gpu is NOT three times the worst case: DELTA_DIFF = 1.5e-6 for position differences and
  DELTA_DIFF_ORI = 3e-6 for orientation differences (changed from the 1e-6 the issue starts from, as it asks when the derivation says so).
- action norms: actions are bit identical; an fp32 sum of 7 squares and a sqrt: 4 * 2^-24 relative.  In dock mode the action is clipped to
  a limit interpolated over the previous position error, which carries EPS_POS times the slope of the interpolation: added to the action
  noise where that interpolation is active (_dynamics_noise).
- dq norms: one rounding of dq_next per joint (|dq| < 0.125: 3.7e-9) -> 8 * 2^-24 relative + 2e-8.
- dynamic step scales (approach dynamic_action_delta_scale, dock dynamic limits) multiply the executed dq by a function of the fp32
  position error: q itself then drifts from the oracle's by dl * slope * EPS_POS per step, accumulated over the episode and carried to the
  pose through the arm's reach (1.5 m per rad).  Only the env-level fuzz configs enable these; for them EPS_POS / EPS_ORI grow with the
  episode step and the tie widths grow with them (never below the constants).
- joint_limit_margin_min = 2 * (q - lower) / span in fp32 from fp32(q): 2 * 2.4e-7 / min span + 4 * 2^-24.

Ties, classified on the reference side only (DELTA_* above; a conjunction is ambiguous iff some term is tied and every other holds):
- state tie: near-goal / pre-near-goal / success gates on (position, orientation) error.  Drops the env for the rest of its episode; it is
  re-admitted at its next reset if both sides finished the episode on the same step with equal RNG words.
- counter tie: prev_in_near and |curr_pos - prev_pos| < DELTA_DIFF.  Taints the drift counter (may differ by the number of such ties in
  the episode) and the components that read it, until the next reset.  Everything else stays compared.
- step tie: every other gate of the two reward functions (STEP_GATES): excuses the components the entry names, on that step.

Bounds of the weighted components: |dev - ref| <= 4 * S_k * eps + 16 * 2^-24 * |ref| + 1e-7, S_k by central differences of kp1o_reward_eval
over every noisy input with half-width h = 4 * eps (so 4 * S_k * eps = |c(x + h) - c(x - h)| / 2), summed over the inputs.  The total reward
is compared on every compared env-step as reward - sum(excused summed components) within the sum of the bounds of the summed components.
"""
from __future__ import annotations

import copy
import json
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from conftest import GOLDEN
from oracle import oracle as orc
from rl_brain_trainer_amd import config as kcfg
from test_env_parity_gpu import _two_float
from route_lockstep import _and_ambiguous

N_ENVS = 200
SEED = 4242
EXTRA_STEPS = 8
U = 2.0 ** -24

DELTA_GATE = 2e-6
DELTA_DIFF = 1.5e-6
DELTA_DIFF_ORI = 3e-6
EPS_POS_ABS, EPS_ORI_ABS = 2.1e-7, 4.2e-7
REACH_M = 1.5

# existing project constants
OBS_TOL, RESET_OBS_TOL, TERMINAL_OBS_TOL = 2e-5, 2e-6, 2e-5
POSE_TOL = 1e-5           # position / orientation error norms (x3 for orientation), raw-error components, q / ee_pose6 rows
F64_REWARD_TOL, F64_OBS_TOL, F64_STATE_TOL = 1e-9, 6e-8, 1e-11
MARGIN = 4.0

# inputs: 3/4 of the envs servo to the goal, 1/4 take uniform actions; the last LIMIT_GROUP envs start next to a joint limit
SERVO = {"approach": (0.8, 0.1), "dock": (0.6, 0.3)}      # gain, +- noise per mode (the drift-counter floor needs the envs to keep moving near the goal)
# With +-0.1 the servoing envs hover about 1 mm from the goal.  A near-goal threshold inside that range is crossed back and forth: per env
# about steps * 2 * DELTA_GATE / range = 90 * 4e-6 / 1e-3 = 36 % state ties.  Cases whose near-goal radius is below 3 mm (4 of the 120
# approach fuzz cases) servo with +-0.8 instead, which hovers at 8 mm and crosses such a radius rarely and fast.
WIDE_NOISE, WIDE_NOISE_BELOW_M = 0.8, 3e-3
UNIFORM = 1.2
LIMIT_GROUP = 16
# thresholds that gate dq_norm / delta_q_change_l2 (fuzzed median 0.55), scaled into the range those reach near the goal under the base
# configs and the servo noise above (median dq_norm 0.0043 in approach mode, 0.0016 in dock mode, delta_q_change_l2 0.0025)
REACHABLE = {"approach": (0.008, ("dock_coarse_ready_dq_threshold", "finisher_ready_dq_threshold")),
             "dock": (0.004, ("dq_penalty_threshold", "delta_q_change_penalty_threshold", "low_motion_dq_threshold"))}

FUZZ_BASE = {"approach": ("workspace_expansion_bigtrain", 5), "dock": ("dock_workspace_handoff_noop_ft_12env_raw", 0)}
SHIPPED = (("workspace_expansion_bigtrain", 5), ("workspace_full_coverage_randomstart_overnight", 10), ("dock_workspace_handoff_noop_ft_12env_raw", 0))
ENV_FUZZ = ("fuzz0_approach", "fuzz1_approach", "fuzz2_approach", "fuzz3_dock", "fuzz4_dock", "fuzz5_dock")


# ============================================================================== cases
@dataclass(frozen=True)
class Case:
    name: str
    base: str
    stage: int
    fuzz_id: int = -1     # index into reward_fuzz.json, -1 = the base config's own reward block


@lru_cache(maxsize=1)
def _fuzz_cases() -> list:
    return json.loads((GOLDEN / "reward_fuzz.json").read_text())["cases"]


@lru_cache(maxsize=1)
def all_cases() -> tuple[Case, ...]:
    out = []
    for k, c in enumerate(_fuzz_cases()):
        base, stage = FUZZ_BASE[c["mode"]]
        out.append(Case(f"fuzz{k:03d}_{c['mode']}", base, stage, k))
    for name in ENV_FUZZ:
        meta = json.loads(str(np.load(GOLDEN / f"trace_{name}.npz")["meta"]))
        out.append(Case(name, name, int(meta["stage"])))
    out += [Case(f"shipped_{name}", name, stage) for name, stage in SHIPPED]
    return tuple(out)


def chunks(size: int = 10) -> list[tuple[Case, ...]]:
    """the cases in chunks of one mode each (the fuzz cases are ordered approach first)"""
    cs = all_cases()
    return [cs[i:i + size] for i in range(0, len(cs), size)]


def config_dict(case: Case) -> dict:
    cfgd = json.loads((GOLDEN / "configs" / f"{case.base}.json").read_text())
    if case.fuzz_id >= 0:
        fc = _fuzz_cases()[case.fuzz_id]
        block = "reward" if fc["mode"] == "approach" else "dock_reward"
        cfgd["env"][block] = dict(fc["config"])
        factor, keys = REACHABLE[fc["mode"]]
        for key in keys:
            cfgd["env"][block][key] = float(cfgd["env"][block][key]) * factor
    return cfgd


def build_config(cfgd: dict) -> kcfg.EnvConfig:
    return kcfg.to_env_config(copy.deepcopy(cfgd), handoff_base_dirs=(GOLDEN,))


def mode_name(cfg: kcfg.EnvConfig) -> str:
    return "dock" if int(cfg.c.env.mode) == kcfg.MODE_NAMES["dock"] else "approach"


# ============================================================================== the gates
def _pos(v):
    return float(v) if v is not None else None


def _if_pos(v):
    """a threshold that switches its clause off when <= 0"""
    return float(v) if v > 0.0 else None


@dataclass(frozen=True)
class Gate:
    """all(quantity_j <= threshold_j); `active` reads the config, `when` names a per-env flag that must hold, `feeds` the components that
    read the gate.  A threshold function returning None drops its term."""
    name: str
    terms: tuple          # ((quantity name, threshold function of the config), ...)
    feeds: tuple
    active: object = None
    when: str = ""


def _pose(prefix: str, pos_field, ori_field, block: str):
    return ((f"{prefix}_pos", lambda c, f=pos_field: _pos(getattr(getattr(c, block), f))),
            (f"{prefix}_ori", lambda c, f=ori_field: _pos(getattr(getattr(c, block), f))))


def _ready_gates(tag: str, stem: str) -> list[Gate]:
    r = "reward"
    enabled = lambda c: getattr(c.reward, f"{stem}_pos_threshold_m") > 0.0 and getattr(c.reward, f"{stem}_ori_threshold_rad") > 0.0
    motion = lambda p: ((f"{p}action_norm", lambda c: _if_pos(getattr(c.reward, f"{stem}_action_threshold"))),
                        (f"{p}dq_norm", lambda c: _if_pos(getattr(c.reward, f"{stem}_dq_threshold"))))
    nh = ("near_handoff_action_penalty", "near_handoff_dq_penalty", "near_handoff_motion_bonus", "near_handoff_settle_bonus")
    return [
        Gate(f"curr_{tag}_pose", _pose("curr", f"{stem}_pos_threshold_m", f"{stem}_ori_threshold_rad", r),
             (f"{stem}_regression_penalty", f"in_{stem}_pose") + nh, enabled),
        Gate(f"prev_{tag}_pose", _pose("prev", f"{stem}_pos_threshold_m", f"{stem}_ori_threshold_rad", r), (f"{stem}_regression_penalty",), enabled),
        Gate(f"curr_{tag}", _pose("curr", f"{stem}_pos_threshold_m", f"{stem}_ori_threshold_rad", r) + motion(""),
             (f"{stem}_bonus", f"{stem}_retention_bonus", f"{stem}_dwell_bonus", f"{stem}_leave_penalty", f"in_{stem}"), enabled),
        Gate(f"prev_{tag}", _pose("prev", f"{stem}_pos_threshold_m", f"{stem}_ori_threshold_rad", r) + motion("prev_"),
             (f"{stem}_bonus", f"{stem}_retention_bonus", f"{stem}_leave_penalty"), enabled),
    ]


def _approach_gates(c) -> list[Gate]:
    r = c.reward
    ho_terms = lambda p: ((f"{p}_pos", lambda c: _pos(c.reward.handover_pos_threshold_m)), (f"{p}_ori", lambda c: _if_pos(c.reward.handover_ori_threshold_rad)))
    ho_on = lambda c: c.reward.handover_pos_threshold_m > 0.0
    nh_on = lambda c: c.reward.near_handoff_pos_threshold_m > 0.0 and c.reward.near_handoff_ori_threshold_rad > 0.0
    g = [Gate(f"milestone{i}", (("curr_ori", lambda c, i=i: float(c.reward.orientation_milestone_thresholds_rad[i])),),
              ("orientation_milestone_bonus",), when="pre") for i in range(int(r.n_orientation_milestones))]
    g += [
        Gate("coarse_orientation", (("curr_ori", lambda c: float(c.reward.coarse_orientation_bonus_threshold_rad)),), ("coarse_orientation_bonus",), when="pre"),
        Gate("curr_handover", ho_terms("curr"), ("handover_bonus", "handover_retention_bonus", "handover_dwell_bonus", "handover_leave_penalty",
                                                 "handover_regression_penalty", "smoothness_penalty", "smoothness_multiplier", "in_handover_zone"), ho_on),
        Gate("prev_handover", ho_terms("prev"), ("handover_bonus", "handover_retention_bonus", "handover_leave_penalty", "handover_regression_penalty",
                                                 "smoothness_penalty", "smoothness_multiplier"), ho_on),
    ]
    g += _ready_gates("dock_coarse", "dock_coarse_ready") + _ready_gates("finisher", "finisher_ready")
    g += [
        Gate("curr_near_handoff", _pose("curr", "near_handoff_pos_threshold_m", "near_handoff_ori_threshold_rad", "reward"),
             ("dock_coarse_ready_regression_penalty", "finisher_ready_regression_penalty", "near_handoff_action_penalty", "near_handoff_dq_penalty",
              "near_handoff_motion_bonus", "near_handoff_settle_bonus", "same_step_alignment_bonus", "in_near_handoff_zone"), nh_on),
        Gate("prev_near_handoff", _pose("prev", "near_handoff_pos_threshold_m", "near_handoff_ori_threshold_rad", "reward"),
             ("dock_coarse_ready_regression_penalty", "finisher_ready_regression_penalty"), nh_on),
        Gate("same_step_signs", (("d_pos", lambda c: 0.0), ("d_ori", lambda c: 0.0)), ("same_step_alignment_bonus",)),
    ]
    return g


def _near_strict(c) -> tuple[float, float]:
    r = c.dock_reward
    return (r.near_strict_pos_threshold_m if r.near_strict_pos_threshold_m != 0.0 else r.tight_pose_pos_threshold_m * 2.0,
            r.near_strict_ori_threshold_rad if r.near_strict_ori_threshold_rad != 0.0 else r.tight_pose_ori_threshold_rad * 3.0)


def _dock_gates(c) -> list[Gate]:
    d = "dock_reward"
    ns = lambda p: ((f"{p}_pos", lambda c: _near_strict(c)[0]), (f"{p}_ori", lambda c: _near_strict(c)[1]))
    basin_on = lambda c: c.dock_reward.basin_outer_radius_m > 0.0 and c.dock_reward.basin_inner_radius_m > 0.0 and c.dock_reward.basin_dwell_radius_m > 0.0
    entry_on = lambda c: c.dock_reward.entry_action_penalty_near_pos_threshold_m > 0.0 and \
        c.dock_reward.entry_action_penalty_far_pos_threshold_m > c.dock_reward.entry_action_penalty_near_pos_threshold_m
    entry_feeds = ("entry_action_penalty_scale", "smoothness_penalty", "action_delta_violation_penalty", "delta_q_change_penalty")
    radius = lambda q, f: ((q, lambda c: max(float(getattr(c.dock_reward, f)), 1e-9)),)
    g = [
        Gate("curr_tight", _pose("curr", "tight_pose_pos_threshold_m", "tight_pose_ori_threshold_rad", d),
             ("tight_pose_bonus", "tight_pose_dwell_bonus", "strict_pose_leave_penalty", "strict_center_reward", "strict_center_small_action_bonus",
              "strict_center_dwell_bonus", "drift_penalty", "smoothness_penalty", "preserve_state_bonus", "strict_hold_bonus", "tiny_correction_bonus",
              "in_tight_pose")),
        Gate("prev_tight", _pose("prev", "tight_pose_pos_threshold_m", "tight_pose_ori_threshold_rad", d), ("strict_pose_leave_penalty", "drift_penalty")),
        Gate("curr_near_strict", ns("curr"), ("preserve_state_bonus", "tiny_correction_bonus", "near_strict_regression_penalty", "aggressive_action_penalty",
                                              "dq_penalty", "in_near_strict")),
        Gate("prev_near_strict", ns("prev"), ("near_strict_regression_penalty",)),
        Gate("convergence_position", (("min_pos", lambda c: float(c.dock_reward.convergence_position_radius_m)),), ("convergence_position_progress",),
             lambda c: c.dock_reward.convergence_position_radius_m > 0.0),
        Gate("convergence_orientation", (("min_ori", lambda c: float(c.dock_reward.convergence_orientation_radius_rad)),), ("convergence_orientation_progress",),
             lambda c: c.dock_reward.convergence_orientation_radius_rad > 0.0),
        Gate("position_first", (("curr_pos", lambda c: float(c.dock_reward.position_first_orientation_pos_threshold_m)),),
             ("convergence_orientation_progress", "orientation_position_gate_scale"), lambda c: c.dock_reward.position_first_orientation_pos_threshold_m > 0.0),
        Gate("entry_penalty_near_end", (("max_pos", lambda c: float(c.dock_reward.entry_action_penalty_near_pos_threshold_m)),), entry_feeds, entry_on),
        Gate("entry_penalty_far_end", (("max_pos", lambda c: float(c.dock_reward.entry_action_penalty_far_pos_threshold_m)),), entry_feeds, entry_on),
        Gate("preserve_tolerances", (("d_entry_pos", lambda c: float(c.dock_reward.preserve_position_tolerance_m)),
                                     ("d_entry_ori", lambda c: float(c.dock_reward.preserve_orientation_tolerance_rad))), ("preserve_state_bonus",),
             lambda c: c.dock_reward.preserve_state_bonus > 0.0),
        Gate("low_motion", ns("curr") + (("action_norm", lambda c: _if_pos(c.dock_reward.low_motion_action_threshold)),
                                         ("dq_norm", lambda c: _if_pos(c.dock_reward.low_motion_dq_threshold))), ("low_motion_bonus",),
             lambda c: c.dock_reward.low_motion_bonus > 0.0),
        Gate("tiny_correction", (("d_pos", lambda c: 0.0), ("d_ori", lambda c: 0.0),
                                 ("action_norm", lambda c: _if_pos(c.dock_reward.tiny_correction_action_threshold))), ("tiny_correction_bonus",),
             lambda c: c.dock_reward.tiny_correction_bonus > 0.0),
    ]
    for zone, f, bonus, leave, extra in (("outer", "basin_outer_radius_m", "basin_outer_bonus", "basin_outer_exit_penalty", ("basin_drift_penalty",)),
                                         ("inner", "basin_inner_radius_m", "basin_inner_bonus", "basin_inner_exit_penalty", ()),
                                         ("dwell", "basin_dwell_radius_m", "basin_dwell_bonus", "basin_dwell_break_penalty", ())):
        g.append(Gate(f"curr_basin_{zone}", radius("curr_pos", f), (bonus, leave, "basin_zone_index") + extra, basin_on))
        g.append(Gate(f"prev_basin_{zone}", radius("prev_pos", f), (leave,) + extra, basin_on))
    return g


def step_gates(cfg: kcfg.EnvConfig) -> list[Gate]:
    """STEP_GATES of the config's mode: the one table the step-tie classification is driven by"""
    return _dock_gates(cfg.c) if mode_name(cfg) == "dock" else _approach_gates(cfg.c)


def state_gates(cfg: kcfg.EnvConfig) -> list[Gate]:
    """near-goal (on the current and the previous pose: prev_in_near is evaluated anew each step, also right after a reset) and success gates;
    both modes read the approach block's near-goal thresholds"""
    near_ori = lambda c: float(c.reward.near_goal_ori_threshold_rad) if c.reward.use_orientation_gate else None
    succ_ori = lambda c: float(c.termination.success_ori_threshold_rad) if c.termination.require_orientation else None
    g = [Gate(f"{p}_near_goal", ((f"{p}_pos", lambda c: float(c.reward.near_goal_pos_threshold_m)), (f"{p}_ori", near_ori)), ()) for p in ("curr", "prev")]
    # success = pose terms and dwell_count >= success_dwell_steps: the integer term is never tied itself, but it has to hold for a tie to matter
    g.append(Gate("success", (("curr_pos", lambda c: float(c.termination.success_pos_threshold_m)), ("curr_ori", succ_ori)), (), when="dwell_reached"))
    return g


# The pre-near-goal gate writes one sticky bit (pre_near_goal_hit) and is otherwise read by this step's reward only.  A tie on it is a state
# tie while the bit is still open; once an earlier, untied step of the episode has set the bit on both sides, a tie can change nothing but
# the step's own components, and is a step tie feeding PRE_FEEDS (approach mode; the dock reward does not read the gate).
def pre_near_gate() -> Gate:
    near_ori = lambda c: float(c.reward.near_goal_ori_threshold_rad) if c.reward.use_orientation_gate else None
    return Gate("curr_pre_near_goal", (("curr_pos", lambda c: float(c.reward.pre_near_goal_pos_threshold_m)), ("curr_ori", near_ori)), PRE_FEEDS)


PRE_FEEDS = ("near_field_orientation_progress", "orientation_progress", "orientation_milestone_bonus", "near_field_orientation_center", "pre_near_goal_bonus",
             "pre_near_to_near_progress", "coarse_orientation_bonus", "same_step_alignment_bonus", "in_pre_near_goal")


# width kind of every gated quantity
_KIND = {"curr_pos": "pos", "prev_pos": "pos", "max_pos": "pos", "min_pos": "pos", "curr_ori": "ori", "prev_ori": "ori", "min_ori": "ori",
         "d_pos": "d_pos", "d_ori": "d_ori", "d_entry_pos": "d_entry_pos", "d_entry_ori": "d_entry_ori",
         "action_norm": "act", "prev_action_norm": "prev_act", "dq_norm": "dq", "prev_dq_norm": "dq"}


def _ambiguous(gate: Gate, c, qty: dict, width: dict) -> np.ndarray | None:
    """bool [...]: can the two precisions disagree on this gate?  None if the config switches it off"""
    if gate.active is not None and not gate.active(c):
        return None
    terms = [(q, fn(c)) for q, fn in gate.terms]
    terms = [(q, thr) for q, thr in terms if thr is not None]
    if not terms:
        return None
    shape = qty[terms[0][0]].shape
    vals = np.stack([qty[q].reshape(-1) for q, _ in terms])
    thrs = np.array([thr for _, thr in terms])
    wid = np.stack([width[_KIND[q]].reshape(-1) for q, _ in terms])
    amb = _and_ambiguous(vals, thrs, wid).reshape(shape)
    if gate.when:
        amb &= qty[gate.when]
    return amb


# ============================================================================== components
EXACT = {"approach": ("near_goal_entry_count", "near_goal_drift_count", "dwell_count", "in_pre_near_goal", "in_near_goal", "in_handover_zone",
                      "in_dock_coarse_ready", "in_dock_coarse_ready_pose", "in_finisher_ready", "in_finisher_ready_pose", "in_near_handoff_zone"),
         "dock": ("basin_zone_index", "dwell_count", "in_tight_pose", "in_near_strict", "near_goal_entry_count", "near_goal_drift_count", "in_near_goal")}
# raw error norms and their differences: POSE_TOL (x3 where an orientation norm enters, as test_step_trace_gpu does)
RAW = {"approach": {"curr_pos_error": 1, "curr_ori_error": 3, "curr_action_norm": 1, "curr_dq_norm": 1},
       "dock": {"curr_pos_error": 1, "curr_ori_error": 3, "entry_pos_error": 1, "entry_ori_error": 3, "entry_action_l2": 1, "entry_dq_norm": 1,
                "entry_to_curr_delta_position_error": 1, "entry_to_curr_delta_orientation_error": 3, "entry_to_curr_delta_action_l2": 1,
                "entry_to_curr_delta_dq_norm": 1}}
# the terms of the reward sum (kp1_oracle.c compute_*_reward); the others only report
NOT_SUMMED = {"approach": ("global_orientation_progress", "near_field_orientation_progress", "near_goal_bonus_scale", "drift_penalty_scale",
                           "smoothness_multiplier"),
              "dock": ("orientation_position_gate_scale", "entry_action_penalty_scale")}
DRIFT_READERS = {"approach": ("drift_penalty", "drift_penalty_scale", "near_goal_drift_count"), "dock": ("near_goal_drift_count",)}


def component_classes(mode: str) -> dict:
    names = orc.component_names(kcfg.MODE_NAMES[mode])
    idx = {n: k for k, n in enumerate(names)}
    exact = np.array([idx[n] for n in EXACT[mode]])
    raw = np.array([idx[n] for n in RAW[mode]])
    raw_factor = np.array([RAW[mode][n] for n in RAW[mode]], dtype=np.float64)
    weighted = np.array([k for k, n in enumerate(names) if n not in EXACT[mode] and n not in RAW[mode]])
    summed = np.array([k for k, n in enumerate(names) if n not in EXACT[mode] and n not in RAW[mode] and n not in NOT_SUMMED[mode]])
    return {"names": names, "idx": idx, "exact": exact, "raw": raw, "raw_factor": raw_factor, "weighted": weighted, "summed": summed,
            "drift": np.array([idx[n] for n in DRIFT_READERS[mode]])}


# ============================================================================== reference pass
def _wrap(x: np.ndarray) -> np.ndarray:
    return (x + np.pi) % (2.0 * np.pi) - np.pi


def _errors(pose: np.ndarray, goal: np.ndarray):
    pe, oe = goal[..., :3] - pose[..., :3], _wrap(goal[..., 3:] - pose[..., 3:])
    return pe, oe, np.linalg.norm(pe, axis=-1), np.linalg.norm(oe, axis=-1)


def step_scale(cfg: kcfg.EnvConfig) -> np.ndarray:
    e = cfg.c.env
    return np.array(cfg.c.joints.delta_limit[:]) * (e.dock_action_delta_scale or e.action_delta_scale)


def limit_group(cfg: kcfg.EnvConfig, n: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(env ids, initial_q [n, 7] with rows of the group inside the outer 10 % of the span of one or two joints, goal_q [n, 7] a centimetre
    further on (as near as the dock mode's own resets put it: a goal across the workspace, or even at the limit itself, puts the dock
    quotient terms at 1e6 - 1e7, where a few fp64 ulps exceed the f64 leg's 1e-9), push [n, 7] in
    {-1, 0, 1}: the action that drives those joints on toward their limit)"""
    lo, hi = np.array(cfg.c.joints.lower[:]), np.array(cfg.c.joints.upper[:])
    span = hi - lo
    rng = np.random.default_rng(777)
    ids = np.arange(n - LIMIT_GROUP, n)
    q0 = np.zeros((n, 7))
    goal = np.zeros((n, 7))
    push = np.zeros((n, 7))
    for k, i in enumerate(ids):
        q = rng.uniform(lo + 0.25 * span, hi - 0.25 * span)
        for j in rng.choice(7, size=1 + k % 2, replace=False):
            side = 1.0 if rng.random() < 0.5 else -1.0
            frac = rng.uniform(0.02, 0.10)
            q[j] = hi[j] - frac * span[j] if side > 0 else lo[j] + frac * span[j]
            push[i, j] = side
        q0[i] = q
        goal[i] = q + rng.uniform(-0.004, 0.004, 7) + 0.01 * push[i]
    return ids, q0, goal, push


def _interp_slope(near_t: float, far_t: float, near_v: float, far_v: float) -> float:
    return abs(far_v - near_v) / (far_t - near_t) if (near_t > 0.0 and far_t > near_t) else 0.0


def _dynamics_noise(cfg: kcfg.EnvConfig, prev_pos: np.ndarray, ep_step: np.ndarray):
    """(extra position noise, extra orientation noise, absolute action noise) [T, N] from the step scales that are functions of the fp32
    position error (module docstring); all zero for configs without dynamic scales"""
    e = cfg.c.env
    dl = np.array(cfg.c.joints.delta_limit[:])
    base = EPS_POS_ABS + 3 * U * prev_pos
    act = np.zeros_like(prev_pos)
    if mode_name(cfg) == "dock":
        nt, ft = e.dock_dynamic_action_limit_near_pos_threshold_m, e.dock_dynamic_action_limit_far_pos_threshold_m
        s_act = _interp_slope(nt, ft, e.dock_dynamic_residual_action_limit_near, e.dock_dynamic_residual_action_limit_far)
        s_dqc = _interp_slope(nt, ft, e.dock_dynamic_delta_q_change_limit_scale_near, e.dock_dynamic_delta_q_change_limit_scale_far)
        inside = (prev_pos > nt - DELTA_GATE) & (prev_pos < ft + DELTA_GATE)
        per_joint = (e.dock_action_delta_scale or e.action_delta_scale) * (s_act + s_dqc)
        act = np.where(inside, np.sqrt(7.0) * s_act * base, 0.0)
    else:
        s = 0.0
        nt = ft = 0.0
        if e.dynamic_action_delta_scale_enabled:
            nt, ft = e.dynamic_action_delta_scale_near_pos_threshold_m, e.dynamic_action_delta_scale_far_pos_threshold_m
            s = _interp_slope(nt, ft, e.dynamic_action_delta_scale_near_multiplier, e.dynamic_action_delta_scale_far_multiplier)
        inside = (prev_pos > nt - DELTA_GATE) & (prev_pos < ft + DELTA_GATE)
        per_joint = e.action_delta_scale * s
    dq_step = np.where(inside, per_joint * base, 0.0) * float(np.sum(dl))      # sum over joints of the per-step q error
    cum = np.zeros_like(dq_step)
    for t in range(dq_step.shape[0]):                                          # accumulated since the episode's start
        cum[t] = dq_step[t] + (np.where(ep_step[t] > 0, cum[t - 1], 0.0) if t else 0.0)
    return REACH_M * cum, cum, act


class Reference:
    """One reference pass; see reference_pass()."""


def reference_pass(cfgd: dict, stage: int, actions: np.ndarray | None = None, n: int = N_ENVS, seed: int = SEED, action_seed: int = 0,
                   classify: bool = True) -> Reference:
    """Step n oracle envs of config dict cfgd; actions [T, n, 7] float32 replays a schedule (the teeth tests), None generates it."""
    cfg = build_config(cfgd)
    mode = mode_name(cfg)
    mode_id = kcfg.MODE_NAMES[mode]
    T = int(cfg.c.termination.max_episode_steps) + EXTRA_STEPS
    cls = component_classes(mode)
    K = len(cls["names"])
    ora = orc.OracleVecEnv(cfg, n, seed0=seed, stage=stage)
    ora.reset()
    ids, q_init, q_goal, push = limit_group(cfg, n)
    for i in ids:
        ora.reset_env(int(i), {"initial_q": q_init[i], "goal_q": q_goal[i]})
    R = Reference()
    R.cfg, R.cfgd, R.stage, R.mode, R.T, R.n, R.seed, R.cls = cfg, cfgd, stage, mode, T, n, seed, cls
    R.limit_ids, R.limit_q, R.limit_goal_q = ids, q_init, q_goal
    q0, stage0 = ora.fields("q", "last_reset_stage")
    # a reset with an explicit initial_q samples no stage: device and oracle report the curriculum stage for it (tests/test_env_control_gpu.py)
    explicit_stage = min(max(int(stage), 0), int(cfg.c.n_stages) - 1)
    stage0[ids] = explicit_stage
    R.reset0 = {"obs": ora.obs.copy(), "rng": ora.rng_words(), "q": q0, "stage": stage0}

    dev = {"obs": np.zeros((T, n, kcfg.OBS_DIM), np.float32), "terminal_obs": np.zeros((T, n, kcfg.OBS_DIM), np.float32),
           "reward": np.zeros((T, n)), "comps": np.zeros((T, n, K)), "done": np.zeros((T, n), np.int64),
           "dwell": np.zeros((T, n), np.int64), "entry": np.zeros((T, n), np.int64), "drift": np.zeros((T, n), np.int64),
           "flags": np.zeros((T, n), np.int64), "step_count": np.zeros((T, n), np.int64), "stage": np.zeros((T, n), np.int64),
           "q": np.zeros((T, n, 7)), "dq": np.zeros((T, n, 7)), "ee": np.zeros((T, n, 6)), "pos_err": np.zeros((T, n)), "ori_err": np.zeros((T, n)),
           "entry_metrics": np.zeros((T, n, 4)), "rng": np.zeros((T, n, 6), np.uint64), "rng_valid": np.zeros(T, bool)}
    pre = {k: np.zeros((T, n, w)) for k, w in (("prev_pose", 6), ("curr_pose", 6), ("goal_pose", 6), ("action", 7), ("prev_action", 7), ("scalars", 8))}
    pre["flags"] = np.zeros((T, n, 7), np.int32)
    pre["ep_step"] = np.zeros((T, n), np.int64)
    pre["drift_pre"] = np.zeros((T, n), np.int64)
    pre["q_reset"] = np.zeros((T, n, 7))
    R.actions = np.zeros((T, n, 7), np.float32) if actions is None else np.ascontiguousarray(actions, dtype=np.float32)
    arng = np.random.default_rng(1000 + action_seed)
    dl = step_scale(cfg)
    gain, noise = SERVO[mode]
    if mode == "approach" and cfg.c.reward.near_goal_pos_threshold_m < WIDE_NOISE_BELOW_M:
        noise = WIDE_NOISE
    pushing = np.zeros(n, bool)
    pushing[ids] = True
    a_r, tc = cfg.c.reward, cfg.c.termination
    for t in range(T):
        q, goal_q, ee_prev, prev_action, dq_prev, goal_pose, ep_step, e_pos, e_ori, e_act, e_dq = ora.fields(
            "q", "goal_q", "ee_pose6", "prev_action", "dq", "goal_pose6", "episode_step", "entry_position_error_norm", "entry_orientation_error_norm",
            "entry_action_l2", "entry_dq_norm")
        if actions is None:
            a = arng.uniform(-UNIFORM, UNIFORM, size=(n, 7))
            servo = gain * (goal_q - q) / dl + arng.uniform(-noise, noise, size=(n, 7))
            a[: 3 * n // 4] = servo[: 3 * n // 4]
            a[pushing] = np.where(push[pushing] != 0.0, push[pushing], servo[pushing])
            R.actions[t] = a.astype(np.float32)
        a64 = R.actions[t].astype(np.float64)
        out = ora.step_out(a64)
        obs_step = ora.obs.copy()
        q1, dq1, ee1, act1, dwell, entry, drift = ora.fields("q", "dq", "ee_pose6", "prev_action", "dwell_count", "near_goal_entry_count", "near_goal_drift_count")
        done = (out["terminated"] != 0) | (out["truncated"] != 0)
        _, _, prev_pos, prev_ori = _errors(ee_prev, goal_pose)
        curr_pos, curr_ori = out["position_error_norm"], out["orientation_error_norm"]
        gate_ori = bool(a_r.use_orientation_gate)
        near = lambda p, o, thr: (p <= thr) & ((o <= a_r.near_goal_ori_threshold_rad) | (not gate_ori))
        pre["flags"][t] = np.stack([near(curr_pos, curr_ori, a_r.pre_near_goal_pos_threshold_m), near(prev_pos, prev_ori, a_r.near_goal_pos_threshold_m),
                                    near(curr_pos, curr_ori, a_r.near_goal_pos_threshold_m), dwell, entry, drift, out["success"]], axis=1)
        pre["scalars"][t] = np.stack([out["joint_limit_margin_min"], out["executed_delta_q_l2"], np.linalg.norm(dq_prev, axis=1), out["delta_q_change_l2"],
                                      e_pos, e_ori, e_act, e_dq], axis=1)
        for key, val in (("prev_pose", ee_prev), ("curr_pose", ee1), ("goal_pose", goal_pose), ("action", act1), ("prev_action", prev_action)):
            pre[key][t] = val
        pre["ep_step"][t] = ep_step
        pre["drift_pre"][t] = drift
        dev["terminal_obs"][t] = obs_step
        dev["reward"][t] = out["reward"]
        dev["comps"][t] = out["components"][:, :K]
        dev["done"][t] = (out["terminated"] != 0) * 1 + (out["truncated"] != 0) * 2 + (out["success"] != 0) * 4
        dev["pos_err"][t], dev["ori_err"][t] = curr_pos, curr_ori
        for i in np.flatnonzero(done):
            ora.reset_env(int(i))
        pushing &= ~done
        dev["obs"][t] = ora.obs
        (dev["q"][t], dev["dq"][t], dev["ee"][t], dev["dwell"][t], dev["entry"][t], dev["drift"][t], dev["step_count"][t], dev["stage"][t], pre_hit, near_hit,
         m0, m1, m2, m3) = ora.fields("q", "dq", "ee_pose6", "dwell_count", "near_goal_entry_count", "near_goal_drift_count", "episode_step", "last_reset_stage",
                                      "pre_near_goal_hit", "near_goal_hit", "entry_position_error_norm", "entry_orientation_error_norm",
                                      "entry_action_l2", "entry_dq_norm")
        dev["flags"][t] = pre_hit + 2 * near_hit
        dev["stage"][t][pushing] = explicit_stage
        dev["entry_metrics"][t] = np.stack([m0, m1, m2, m3], axis=1)
        pre["q_reset"][t] = dev["q"][t]
        if done.any() or t == T - 1:
            dev["rng"][t] = ora.rng_words()
            dev["rng_valid"][t] = True
    R.dev, R.pre = dev, pre
    R.done = (dev["done"] & 3) != 0
    if classify:
        _classify(R)
    return R


def _eval(R: Reference, **over) -> np.ndarray:
    """kp1o_reward_eval on every env-step of the pass with some arguments replaced -> components [T * n, K]"""
    p = R.pre
    arg = {k: (over[k] if k in over else p[k]).reshape(R.T * R.n, -1) for k in ("prev_pose", "curr_pose", "goal_pose", "action", "prev_action", "flags", "scalars")}
    _, c = orc.reward_eval_batch(R.cfg, kcfg.MODE_NAMES[R.mode], arg["prev_pose"], arg["curr_pose"], arg["goal_pose"], arg["action"], arg["prev_action"],
                                 arg["flags"], arg["scalars"])
    return c


def _classify(R: Reference) -> None:
    """noise model, tie classes and component bounds of a reference pass (all from the reference's own values)"""
    cfg, p, T, n, cls = R.cfg, R.pre, R.T, R.n, R.cls
    c = cfg.c
    K = len(cls["names"])
    ppe, poe, prev_pos, prev_ori = _errors(p["prev_pose"], p["goal_pose"])
    cpe, coe, curr_pos, curr_ori = _errors(p["curr_pose"], p["goal_pose"])
    assert np.max(np.abs(curr_pos - R.dev["pos_err"])) <= 1e-12 and np.max(np.abs(curr_ori - R.dev["ori_err"])) <= 1e-12
    # the reconstruction of the reward function's arguments reproduces the oracle's own step
    base = _eval(R).reshape(T, n, K)
    R.reconstruction_error = float(np.max(np.abs(base - R.dev["comps"]) / np.maximum(1.0, np.abs(R.dev["comps"]))))
    assert R.reconstruction_error <= 1e-12, R.reconstruction_error

    ep = p["ep_step"]
    xp, xo, act_abs = _dynamics_noise(cfg, prev_pos, ep)
    # noise of the pose-error norms: the drift of q accumulated up to and including this step for curr, up to the last one for prev
    first = ep == 0
    xp_prev = np.where(first, 0.0, np.concatenate([np.zeros((1, n)), xp[:-1]]))
    xo_prev = np.where(first, 0.0, np.concatenate([np.zeros((1, n)), xo[:-1]]))
    eps = {"curr_pos": EPS_POS_ABS + 3 * U * curr_pos + xp, "prev_pos": EPS_POS_ABS + 3 * U * prev_pos + xp_prev,
           "curr_ori": EPS_ORI_ABS + 3 * U * curr_ori + xo, "prev_ori": EPS_ORI_ABS + 3 * U * prev_ori + xo_prev}
    action_norm, prev_action_norm = np.linalg.norm(p["action"], axis=-1), np.linalg.norm(p["prev_action"], axis=-1)
    prev_act_abs = np.where(first, 0.0, np.concatenate([np.zeros((1, n)), act_abs[:-1]]))
    eps["action"] = 4 * U * action_norm + act_abs
    eps["prev_action"] = 4 * U * prev_action_norm + prev_act_abs
    s = p["scalars"]
    lo, hi = np.array(c.joints.lower[:]), np.array(c.joints.upper[:])
    eps_scalar = [np.full((T, n), 2 * 2.4e-7 / float(np.min(hi - lo)) + 4 * U),                    # joint_limit_margin_min
                  8 * U * s[..., 1] + 2e-8 + _dq_extra(xo, xo_prev), 8 * U * s[..., 2] + 2e-8 + _dq_extra(xo_prev, xo_prev),
                  16 * U * s[..., 3] + 4e-8 + 2 * _dq_extra(xo, xo_prev),                          # dq, prev dq, dq change
                  EPS_POS_ABS + 3 * U * s[..., 4], EPS_ORI_ABS + 3 * U * s[..., 5], 4 * U * s[..., 6], 8 * U * s[..., 7] + 2e-8]   # entry metrics
    R.eps = eps

    R.eps_scalar, R.errors = eps_scalar, {"curr": (cpe, coe), "prev": (ppe, poe)}
    R.fd = R.bound = None

    # ---- ties
    width = {"pos": np.maximum(DELTA_GATE, 3 * np.maximum(eps["curr_pos"], eps["prev_pos"])),
             "ori": np.maximum(DELTA_GATE, 3 * np.maximum(eps["curr_ori"], eps["prev_ori"])),
             "d_pos": np.maximum(DELTA_DIFF, 3 * (eps["curr_pos"] + eps["prev_pos"] - 2 * EPS_POS_ABS + 4.2e-7) * (xp > 0)),
             "d_ori": np.maximum(DELTA_DIFF_ORI, 3 * (eps["curr_ori"] + eps["prev_ori"] - 2 * EPS_ORI_ABS + 8.3e-7) * (xo > 0)),
             "d_entry_pos": np.maximum(DELTA_GATE, 3 * (eps["curr_pos"] + eps_scalar[4])),
             "d_entry_ori": np.maximum(DELTA_DIFF_ORI, 3 * (eps["curr_ori"] + eps_scalar[5])),
             "act": np.maximum(DELTA_GATE, 3 * eps["action"]), "prev_act": np.maximum(DELTA_GATE, 3 * eps["prev_action"]),
             "dq": np.maximum(DELTA_GATE, 3 * np.maximum(eps_scalar[1], eps_scalar[2]))}
    R.width = width
    qty = {"curr_pos": curr_pos, "prev_pos": prev_pos, "curr_ori": curr_ori, "prev_ori": prev_ori, "max_pos": np.maximum(prev_pos, curr_pos),
           "min_pos": np.minimum(prev_pos, curr_pos), "min_ori": np.minimum(prev_ori, curr_ori), "d_pos": curr_pos - prev_pos, "d_ori": curr_ori - prev_ori,
           "d_entry_pos": curr_pos - s[..., 4], "d_entry_ori": curr_ori - s[..., 5], "action_norm": action_norm, "prev_action_norm": prev_action_norm,
           "dq_norm": s[..., 1], "prev_dq_norm": s[..., 2], "pre": p["flags"][..., 0] != 0,
           "dwell_reached": p["flags"][..., 3] >= int(c.termination.success_dwell_steps)}
    R.qty = qty
    state = np.zeros((T, n), bool)
    for g in state_gates(cfg):
        amb = _ambiguous(g, c, qty, width)
        if amb is not None:
            state |= amb
    excused = np.zeros((T, n, K), bool)
    R.gate_ties = {}
    amb_pre = _ambiguous(pre_near_gate(), c, qty, width)
    sure = qty["pre"] & ~amb_pre
    had = np.zeros((T, n), bool)               # an earlier untied step of this episode was inside the pre-near zone
    for t in range(1, T):
        had[t] = (had[t - 1] | sure[t - 1]) & (ep[t] > 0)
    state |= amb_pre & ~had
    R.gate_ties["curr_pre_near_goal"] = int((amb_pre & had).sum())
    if R.mode == "approach":
        for name in PRE_FEEDS:
            excused[..., cls["idx"][name]] |= amb_pre & had
    R.state_tie = state
    for g in step_gates(cfg):
        amb = _ambiguous(g, c, qty, width)
        if amb is None:
            continue
        R.gate_ties[g.name] = int(amb.sum())
        for name in g.feeds:
            excused[..., cls["idx"][name]] |= amb
    R.excused = excused
    R.counter_tie = (p["flags"][..., 1] != 0) & (np.abs(curr_pos - prev_pos) < width["d_pos"])

    # the dq clause of the readiness / low-motion gates, where the pose and action clauses hold (so that it decides the gate)
    R.dq_clause = {}
    if R.mode == "approach":
        for stem in ("dock_coarse_ready", "finisher_ready"):
            thr = getattr(c.reward, f"{stem}_dq_threshold")
            at = getattr(c.reward, f"{stem}_action_threshold")
            pt, ot = getattr(c.reward, f"{stem}_pos_threshold_m"), getattr(c.reward, f"{stem}_ori_threshold_rad")
            if thr > 0.0 and pt > 0.0 and ot > 0.0:
                rest = (curr_pos <= pt) & (curr_ori <= ot) & ((at <= 0.0) | (action_norm <= at))
                R.dq_clause[f"{stem}_dq_threshold"] = (rest & (s[..., 1] <= thr), rest & (s[..., 1] > thr))
    else:
        r = c.dock_reward
        if r.low_motion_bonus > 0.0 and r.low_motion_dq_threshold > 0.0:
            ns_pos, ns_ori = _near_strict(c)
            rest = (curr_pos <= ns_pos) & (curr_ori <= ns_ori) & ((r.low_motion_action_threshold <= 0.0) | (action_norm <= r.low_motion_action_threshold))
            R.dq_clause["low_motion_dq_threshold"] = (rest & (s[..., 1] <= r.low_motion_dq_threshold), rest & (s[..., 1] > r.low_motion_dq_threshold))


def add_bounds(R: Reference) -> None:
    """bounds of the weighted components of a classified pass (module docstring), computed once, when a comparison needs them"""
    if R.bound is not None:
        return
    p, T, n, eps, s = R.pre, R.T, R.n, R.eps, R.pre["scalars"]
    K = len(R.cls["names"])
    (cpe, coe), (ppe, poe) = R.errors["curr"], R.errors["prev"]
    eps_scalar = R.eps_scalar
    # central differences, half-width 4 * eps per input
    fd = np.zeros((T * n, K))

    def central(**kw_pair):
        plus = {k: v[0] for k, v in kw_pair.items()}
        minus = {k: v[1] for k, v in kw_pair.items()}
        return np.abs(_eval(R, **plus) - _eval(R, **minus)) / 2.0

    def unit(v):
        nrm = np.linalg.norm(v, axis=-1, keepdims=True)
        u = np.where(nrm > 1e-12, v / np.maximum(nrm, 1e-300), 0.0)
        u[..., 0] = np.where(nrm[..., 0] > 1e-12, u[..., 0], 1.0)
        return u

    for key, pe, oe in (("curr", cpe, coe), ("prev", ppe, poe)):
        for part, err, sl in (("pos", pe, slice(0, 3)), ("ori", oe, slice(3, 6))):
            h = MARGIN * eps[f"{key}_{part}"][..., None] * unit(err)
            up, dn = p[f"{key}_pose"].copy(), p[f"{key}_pose"].copy()
            up[..., sl] -= h          # moving the pose against the error vector lengthens the error
            dn[..., sl] += h
            fd += central(**{f"{key}_pose": (up, dn)})
    for key in ("action", "prev_action"):
        nrm = np.linalg.norm(p[key], axis=-1)
        rel = (MARGIN * eps[key] / np.maximum(nrm, 1e-12))[..., None]
        fd += central(**{key: (p[key] * (1 + rel), p[key] * (1 - rel))})
    for j, e_j in enumerate(eps_scalar):
        up, dn = s.copy(), s.copy()
        up[..., j] += MARGIN * e_j
        dn[..., j] -= MARGIN * e_j
        fd += central(scalars=(up, dn))
    fd = fd.reshape(T, n, K)
    R.fd = fd
    R.bound = fd + 16 * U * np.abs(R.dev["comps"]) + 1e-7


def _dq_extra(x_now: np.ndarray, x_before: np.ndarray) -> np.ndarray:
    """noise of a dq norm from the drift of q under dynamic step scales: dq_next = q_next - q, the per-step increment of the accumulated drift"""
    return np.abs(x_now - x_before)


# ============================================================================== device-layout arrays
DEVICE_KEYS = ("obs", "terminal_obs", "reward", "comps", "done", "dwell", "entry", "drift", "flags", "step_count", "stage", "q", "dq", "ee", "pos_err",
               "ori_err", "entry_metrics", "rng", "rng_valid", "q_exact")


def as_device(R: Reference, f32: bool = True) -> tuple[dict, dict]:
    """(reset0, per-step arrays) of a reference pass in the layout the comparator takes from a device; f32 rounds the float outputs through
    float32 the way the fp32 handle stores them (q as a two-float pair)"""
    r32 = (lambda x: x.astype(np.float32).astype(np.float64)) if f32 else (lambda x: x)
    dev = {k: (r32(v) if v.dtype == np.float64 and k != "q" else v.copy()) for k, v in R.dev.items()}
    dev["q"] = _two_float(R.dev["q"]) if f32 else R.dev["q"].copy()
    dev["q_exact"] = dev["q"].copy()       # the host copy of q (all 48 bits of the pair); a device fills it on the rng_valid steps
    reset0 = dict(R.reset0)
    reset0["q"] = _two_float(R.reset0["q"]) if f32 else R.reset0["q"]
    return reset0, dev


# ============================================================================== comparator
class Mismatch(AssertionError):
    pass


class Report:
    def __init__(self, K: int) -> None:
        self.worst: dict[str, float] = {}        # worst |device - reference| per quantity
        self.ratio: dict[str, float] = {}        # worst error / bound per quantity
        self.where: dict[str, tuple] = {}
        self.counts: dict[str, int] = {}
        self.nonzero = np.zeros(K, np.int64)     # compared, non-excused env-steps with a non-zero reference component
        self.dq_clause: dict[str, list[int]] = {}

    def add(self, key: str, n: int = 1) -> None:
        self.counts[key] = self.counts.get(key, 0) + int(n)

    def summary(self) -> dict:
        return {"worst": {k: float(f"{v:.3g}") for k, v in sorted(self.worst.items())},
                "ratio": {k: float(f"{v:.3g}") for k, v in sorted(self.ratio.items())}, "counts": dict(sorted(self.counts.items()))}


def compare(R: Reference, reset0: dict, dev: dict, strict: bool = False, label: str = "", bounds: bool = True) -> Report:
    """Assert everything the module docstring lists for a device pass against reference pass R; raises Mismatch naming quantity, step, env and
    component.  strict = the f64 leg: no ties, exact counters, the f64 constants; bounds=False leaves out the
    weighted components and the reward (the reference-only floors do not need their bounds).  Knows nothing about where the device arrays came from."""
    T, n, cls, ref = R.T, R.n, R.cls, R.dev
    if not strict and bounds:
        add_bounds(R)
    names = cls["names"]
    K = len(names)
    rep = Report(K)

    def check(key: str, err: np.ndarray, bound, ctx: tuple, idx=None, comp=None) -> None:
        if err.size == 0:
            return
        err = np.abs(err)
        bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
        ratio = err / bound
        k = int(np.argmax(ratio))
        rep.worst[key] = max(rep.worst.get(key, 0.0), float(err.max()))
        if float(ratio.flat[k]) >= rep.ratio.get(key, -1.0):
            rep.ratio[key] = float(ratio.flat[k])
            pos = np.unravel_index(k, err.shape)
            rep.where[key] = (label, ctx, "env", int(idx[pos[0]]) if idx is not None else None, names[comp[pos[1]]] if comp is not None and len(pos) > 1 else None)
        if float(ratio.flat[k]) > 1.0:
            pos = np.unravel_index(k, err.shape)
            raise Mismatch((label, key, ctx, "env", int(idx[pos[0]]) if idx is not None else None,
                            "component", names[comp[pos[1]]] if comp is not None and len(pos) > 1 else None,
                            "error", float(err.flat[k]), "bound", float(bound.flat[k])))

    def exact(key: str, a: np.ndarray, b: np.ndarray, ctx: tuple, idx: np.ndarray) -> None:
        bad = np.flatnonzero(np.any((a != b).reshape(a.shape[0], -1), axis=1)) if a.size else np.array([], int)
        if bad.size:
            raise Mismatch((label, key, ctx, "envs", idx[bad[:8]].tolist(), "device", a[bad[:4]].tolist(), "reference", b[bad[:4]].tolist()))

    every = np.arange(n)
    ftol = F64_STATE_TOL if strict else POSE_TOL
    # ---- the initial reset (all envs, then the limit group through reset(options=, mask=))
    exact("reset rng", reset0["rng"], R.reset0["rng"], ("reset",), every)
    exact("reset stage", reset0["stage"], R.reset0["stage"], ("reset",), every)
    exact("reset q", reset0["q"], R.reset0["q"] if strict else _two_float(R.reset0["q"]), ("reset",), every)
    check("reset_obs", reset0["obs"].astype(np.float64) - R.reset0["obs"], F64_OBS_TOL if strict else RESET_OBS_TOL, ("reset",), every)

    alive = np.ones(n, bool)
    drift_ties = np.zeros(n, np.int64)          # counter ties so far in the episode
    episode = np.zeros(n, np.int64)             # index of the env's current episode
    clean_first = 0
    summed = np.zeros(K, bool)
    summed[cls["summed"]] = True
    weighted = np.zeros(K, bool)
    weighted[cls["weighted"]] = True
    for key in R.dq_clause:
        rep.dq_clause[key] = [0, 0]
    for t in range(T):
        ctx = ("step", t)
        if not strict:
            alive &= ~R.state_tie[t]
            drift_ties += R.counter_tie[t]
        s = np.flatnonzero(alive)
        done_ref = R.done[t]
        done_dev = (dev["done"][t] & 3) != 0
        exact("done bits", dev["done"][t][s] & 7, ref["done"][t][s] & 7, ctx, s)
        go, fin = s[~done_ref[s]], s[done_ref[s]]
        for key in ("dwell", "entry", "step_count", "stage"):
            exact(key, dev[key][t][s], ref[key][t][s], ctx, s)
        exact("flags", dev["flags"][t][s] & 3, ref["flags"][t][s] & 3, ctx, s)
        tainted = (drift_ties > 0) & (not strict)
        clean = s[~tainted[s]]
        exact("drift counter", dev["drift"][t][clean], ref["drift"][t][clean], ctx, clean)
        loose = go[tainted[go]]
        if loose.size and np.any(np.abs(dev["drift"][t][loose] - ref["drift"][t][loose]) > drift_ties[loose]):
            raise Mismatch((label, "drift counter beyond its ties", ctx, loose[:8].tolist()))
        # ---- continuous state and observations
        check("obs", dev["obs"][t][go].astype(np.float64) - ref["obs"][t][go], F64_OBS_TOL if strict else OBS_TOL, ctx, go)
        check("terminal_obs", dev["terminal_obs"][t][fin].astype(np.float64) - ref["terminal_obs"][t][fin], F64_OBS_TOL if strict else TERMINAL_OBS_TOL, ctx, fin)
        check("reset_obs", dev["obs"][t][fin].astype(np.float64) - ref["obs"][t][fin], F64_OBS_TOL if strict else RESET_OBS_TOL, ctx, fin)
        check("q", dev["q"][t][go] - ref["q"][t][go], ftol, ctx, go)
        check("dq", dev["dq"][t][go] - ref["dq"][t][go], ftol, ctx, go)
        d = np.abs(dev["ee"][t][s] - ref["ee"][t][s])
        d[:, 3:] = np.abs(_wrap(d[:, 3:]))
        check("ee_pose6", d, ftol, ctx, s)
        check("entry_metrics", dev["entry_metrics"][t][s] - ref["entry_metrics"][t][s], ftol * np.array([1, 3, 1, 1]), ctx, s)
        check("position_error_norm", dev["pos_err"][t][s] - ref["pos_err"][t][s], ftol, ctx, s)
        check("orientation_error_norm", dev["ori_err"][t][s] - ref["ori_err"][t][s], ftol * (1 if strict else 3), ctx, s)
        if ref["rng_valid"][t]:
            if not dev["rng_valid"][t]:
                raise Mismatch((label, "device RNG words missing", ctx))
            exact("q after reset", dev["q_exact"][t][fin], ref["q"][t][fin] if strict else _two_float(ref["q"][t][fin]), ctx, fin)
            who = fin if t < T - 1 else s
            exact("rng words", dev["rng"][t][who], ref["rng"][t][who], ctx, who)
        # ---- reward and components
        cd, cr = dev["comps"][t][s], ref["comps"][t][s]
        if strict:
            check("components", cd - cr, F64_REWARD_TOL, ctx, s, np.arange(K))
            check("reward", dev["reward"][t][s] - ref["reward"][t][s], F64_REWARD_TOL, ctx, s)
            skip = np.zeros((s.size, K), bool)
        else:
            skip = R.excused[t][s].copy()
            skip[:, cls["drift"]] |= tainted[s][:, None]
            ok = ~skip
            e_idx = cls["exact"]
            bad = (cd[:, e_idx] != cr[:, e_idx]) & ok[:, e_idx]
            if bad.any():
                i, k = np.argwhere(bad)[0]
                raise Mismatch((label, "indicator component", ctx, "env", int(s[i]), names[e_idx[k]], float(cd[i, e_idx[k]]), float(cr[i, e_idx[k]])))
            r_idx = cls["raw"]
            check("raw_error_components", np.where(ok[:, r_idx], cd[:, r_idx] - cr[:, r_idx], 0.0), POSE_TOL * cls["raw_factor"], ctx, s, r_idx)
            w_idx, sm = cls["weighted"], cls["summed"]
            if bounds:
                check("weighted_components", np.where(ok[:, w_idx], cd[:, w_idx] - cr[:, w_idx], 0.0), R.bound[t][s][:, w_idx], ctx, s, w_idx)
                part_dev = dev["reward"][t][s] - np.sum(np.where(skip[:, sm], cd[:, sm], 0.0), axis=1)
                part_ref = ref["reward"][t][s] - np.sum(np.where(skip[:, sm], cr[:, sm], 0.0), axis=1)
                present = ok[:, sm] & ((cr[:, sm] != 0.0) | (R.fd[t][s][:, sm] > 0.0))
                check("reward", part_dev - part_ref, np.sum(np.where(present, R.bound[t][s][:, sm], 0.0), axis=1) + 1e-7, ctx, s)
        rep.nonzero += np.sum((cr != 0.0) & ~skip, axis=0)
        rep.add("pairs", s.size * K)
        rep.add("excused_pairs", int(skip.sum()))
        rep.add("env_steps", s.size)
        for key, (below, above) in R.dq_clause.items():
            rep.dq_clause[key][0] += int(below[t][s].sum())
            rep.dq_clause[key][1] += int(above[t][s].sum())
        # ---- episode ends
        first = fin[episode[fin] == 0]
        rep.add("first_resets_compared", first.size)
        clean_first += int(np.sum(~tainted[first]))
        rep.add("success_terminations_compared", int(np.sum((ref["done"][t][fin] & 5) == 5)))
        if not strict and ref["rng_valid"][t]:
            # a dropped env comes back if both sides ended the episode here and drew the same reset
            back = np.flatnonzero(~alive & done_ref & done_dev)
            back = back[np.all(dev["rng"][t][back] == ref["rng"][t][back], axis=1)]
            alive[back] = True
            rep.add("readmitted", back.size)
        every_done = np.flatnonzero(done_ref)
        drift_ties[every_done] = 0
        episode[every_done] += 1
    rep.counts.setdefault("readmitted", 0)
    rep.counts["dropped_at_end"] = int(n - alive.sum())
    rep.counts["state_tied_envs"] = int(np.any(R.state_tie, axis=0).sum()) if not strict else 0
    rep.counts["drift_clean_first_episodes"] = clean_first
    rep.counts["counter_ties"] = int(R.counter_tie.sum())
    rep.counts["envs_reset"] = int(np.sum(episode >= 1))
    return rep


def check_case_floors(R: Reference, rep: Report) -> None:
    """the per-case caps and floors (the cross-case ones are summed by the test modules)"""
    n = R.n
    c = rep.counts
    assert c["envs_reset"] == n, ("not every env went through an auto-reset", c["envs_reset"])
    assert c["state_tied_envs"] <= n // 20, ("state-tied envs", c["state_tied_envs"])
    assert c["dropped_at_end"] <= n // 20, ("dropped envs", c["dropped_at_end"])
    assert c["drift_clean_first_episodes"] >= n // 2, ("first episodes with an untainted drift counter", c["drift_clean_first_episodes"])
    assert c["first_resets_compared"] >= 0.9 * n, ("first auto-resets compared", c["first_resets_compared"])
    assert c["excused_pairs"] < 0.02 * c["pairs"], ("excused env-step x component pairs", c["excused_pairs"], c["pairs"])
    if R.cfg.c.termination.terminate_on_success:
        assert c["success_terminations_compared"] >= 20, ("terminated-on-success episodes compared", c["success_terminations_compared"])


class Totals:
    """sums over cases for the cross-case floors: every component non-zero on >= 50 compared, non-excused env-steps in >= 5 cases, and the dq
    clause of every readiness / low-motion gate seen with both values under the same floor"""

    def __init__(self) -> None:
        self.steps: dict[tuple, int] = {}
        self.cases: dict[tuple, int] = {}

    def add(self, R: Reference, rep: Report) -> None:
        for k, name in enumerate(R.cls["names"]):
            self._add((R.mode, name), int(rep.nonzero[k]))
        for key, (below, above) in rep.dq_clause.items():
            self._add((R.mode, key, "holds"), below)
            self._add((R.mode, key, "fails"), above)

    def _add(self, key: tuple, count: int) -> None:
        self.steps[key] = self.steps.get(key, 0) + count
        self.cases[key] = self.cases.get(key, 0) + (count > 0)

    def expected_keys(self) -> list[tuple]:
        keys = [(m, name) for m in ("approach", "dock") for name in orc.component_names(kcfg.MODE_NAMES[m])]
        for m, (_, fields) in REACHABLE.items():
            keys += [(m, f, v) for f in fields if f.endswith("ready_dq_threshold") or f == "low_motion_dq_threshold" for v in ("holds", "fails")]
        return keys

    def short(self) -> list[tuple]:
        return [(k, self.steps.get(k, 0), self.cases.get(k, 0)) for k in self.expected_keys() if self.steps.get(k, 0) < 50 or self.cases.get(k, 0) < 5]
