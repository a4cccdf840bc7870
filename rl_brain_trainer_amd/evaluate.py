"""Deterministic Approach -> Finisher evaluation, batched on the GPU.

Mirrors the reference's serial evaluators (one env + batch-1 ``model.predict`` per episode) as one batched state
machine over all episodes of all stages:

* ``build_curriculum_local_eval_suite``   kinematic_phase1/eval/fixed_eval_suite.py:78-105
* ``dock_coarse_ready`` / ``finisher_ready`` eval_three_stage.py:41-56, eval_approach_finisher.py:24-32
* ``run_approach_with_handoff``           eval_pipeline_ablation.py:60-147
* ``run_policy`` (finisher episode)       eval_three_stage.py:59-125, reset from ``_state_reset_options`` :30-38
* ``evaluate_workspace_expansion``        eval_workspace_expansion.py:86-211 (same stage_metrics / selection JSON)
* ``gated_score`` & friends               workspace/workspace_curriculum.py:10-95

Suites are drawn on the host with numpy's PCG64 exactly like the reference (``default_rng(seed + 1009 * stage)``); the
goal poses come from the fp64 HIP FK kernel.
"""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path
from typing import Any, Callable

import numpy as np
import torch

from . import config as kcfg
from . import native
from .vec_env import ArmKinematicVecEnv, fk_pose6

PolicyFn = Callable[[torch.Tensor], torch.Tensor]  # obs [E, stride] -> clipped deterministic action [E, 7]


# ----------------------------------------------------------------------------- gate scoring (host logic)
# The YAML ``gate:`` block and the ``best_model_selection`` JSON are schemas other tools read (check_workspace_expansion_status.sh,
# plot_workspace_expansion.py): key names and default values are the reference's (workspace/workspace_curriculum.py:20-32).  The
# evaluation itself works on one small numeric table per call instead of walking dicts stage by stage.
_GATE_DEFAULTS: dict[str, Any] = {
    "retention_stage0_4_success": 0.95, "retention_stage5_success": 0.85, "retention_stage_thresholds": (),
    "promotion_stage_success": 0.80, "promotion_ready_rate": 0.80, "max_mean_position_error_m": 0.020, "max_mean_orientation_error_rad": 0.15,
    "score_current_success_weight": 0.45, "score_current_ready_weight": 0.20, "score_retention_weight": 0.20, "score_error_weight": 0.15,
}
_METRIC_COLUMNS = ("success_rate", "finisher_ready_hit_rate", "mean_final_position_error", "mean_final_orientation_error")


class WorkspaceGate:
    """Thresholds and score weights of the workspace-expansion eval gate (attribute per YAML key)."""

    def __init__(self, **overrides: Any) -> None:
        for key, default in _GATE_DEFAULTS.items():
            value = overrides.get(key, default)
            setattr(self, key, tuple(float(v) for v in value) if key == "retention_stage_thresholds" else float(value))

    def as_dict(self) -> dict[str, Any]:
        return {k: getattr(self, k) for k in _GATE_DEFAULTS}


WorkspaceGateConfig = WorkspaceGate   # name the trainers import


def gate_config_from_dict(payload: dict[str, Any] | None) -> WorkspaceGate:
    return WorkspaceGate(**{k: v for k, v in dict(payload or {}).items() if k in _GATE_DEFAULTS})


class _StageTable:
    """stage_metrics {stage index -> summary dict} as columns: `idx` sorted ascending, one float column per gate metric."""

    def __init__(self, stage_metrics: dict[int, dict[str, Any]], missing: tuple[float, float, float, float]) -> None:
        self.idx = np.array(sorted(int(k) for k in stage_metrics), dtype=np.int64)
        rows = [[float(stage_metrics[int(i)].get(name, fill)) for name, fill in zip(_METRIC_COLUMNS, missing)] for i in self.idx]
        self.col = np.array(rows, dtype=np.float64).reshape(len(rows), len(_METRIC_COLUMNS))

    def lookup(self, stages: np.ndarray, column: int, fill: float) -> np.ndarray:
        """column values at the given stage indices; stages without a row read as `fill`"""
        out = np.full(len(stages), fill, dtype=np.float64)
        if self.idx.size:
            pos = np.searchsorted(self.idx, stages)
            hit = (pos < self.idx.size) & (self.idx[np.minimum(pos, self.idx.size - 1)] == stages)
            out[hit] = self.col[pos[hit], column]
        return out


def _passed_mask(tab: _StageTable, gate: WorkspaceGate) -> np.ndarray:
    """per evaluated stage: success, ready-hit rate and both mean errors inside the promotion thresholds"""
    c = tab.col
    return (c[:, 0] >= gate.promotion_stage_success) & (c[:, 1] >= gate.promotion_ready_rate) & \
           (c[:, 2] <= gate.max_mean_position_error_m) & (c[:, 3] <= gate.max_mean_orientation_error_rad)


def stage_passed(metrics: dict[str, Any], gate: WorkspaceGate) -> bool:
    return bool(_passed_mask(_StageTable({0: metrics}, (0.0, 0.0, 999.0, 999.0)), gate)[0])


def retention_ok(stage_metrics: dict[int, dict[str, Any]], gate: WorkspaceGate) -> bool:
    """old stages must keep their success rate: per-stage thresholds where the config lists them (only stages that were evaluated count),
    else stages 0-4 and stage 5 against the two fixed levels (a stage that was not evaluated counts as 0)"""
    tab = _StageTable(stage_metrics, (0.0, 0.0, 999.0, 999.0))
    if gate.retention_stage_thresholds:
        thr = np.asarray(gate.retention_stage_thresholds, dtype=np.float64)
        listed = tab.idx[(tab.idx >= 0) & (tab.idx < thr.size)]
        return bool(np.all(tab.lookup(listed, 0, 0.0) >= thr[listed]))
    succ = tab.lookup(np.arange(6), 0, 0.0)
    return bool(np.all(succ[:5] >= gate.retention_stage0_4_success) and succ[5] >= gate.retention_stage5_success)


def highest_passed_stage(stage_metrics: dict[int, dict[str, Any]], gate: WorkspaceGate) -> int:
    """largest passing stage index below the first FAILING expansion stage (index >= 6); -1 when none passes"""
    tab = _StageTable(stage_metrics, (0.0, 0.0, 999.0, 999.0))
    ok = _passed_mask(tab, gate)
    blockers = np.flatnonzero(~ok & (tab.idx >= 6))
    reach = int(blockers[0]) if blockers.size else tab.idx.size
    good = tab.idx[:reach][ok[:reach]]
    return int(good[-1]) if good.size else -1


def gated_score(stage_metrics: dict[int, dict[str, Any]], current_stage: int, gate: WorkspaceGate) -> dict[str, Any]:
    """best-checkpoint score of one evaluation: weighted current-stage success / ready-hit rate, retention over stages 0..min(5, current)
    and an error score; the current stage's missing errors count as 1.0 (m / rad)"""
    tab = _StageTable(stage_metrics, (0.0, 0.0, 1.0, 1.0))
    stage = np.array([int(current_stage)])
    cur_succ, cur_ready, cur_pos, cur_ori = (float(tab.lookup(stage, k, fill)[0]) for k, fill in enumerate((0.0, 0.0, 1.0, 1.0)))
    kept = tab.lookup(np.arange(0, min(6, int(current_stage) + 1)), 0, 0.0)
    retention = float(kept.sum() / kept.size) if kept.size else 0.0
    limits = np.maximum([gate.max_mean_position_error_m, gate.max_mean_orientation_error_rad], 1e-6)
    error_score = float(0.5 * np.maximum(0.0, 1.0 - np.array([cur_pos, cur_ori]) / limits).sum())
    score = cur_succ * gate.score_current_success_weight + cur_ready * gate.score_current_ready_weight \
        + retention * gate.score_retention_weight + error_score * gate.score_error_weight
    return {
        "score": float(score), "current_stage": int(current_stage), "retention_ok": retention_ok(stage_metrics, gate),
        "highest_passed_stage": highest_passed_stage(stage_metrics, gate), "current_stage_success_rate": cur_succ,
        "current_stage_ready_rate": cur_ready, "retention_mean_success_rate": retention, "error_score": error_score,
    }


# ----------------------------------------------------------------------------- suites
def build_curriculum_local_eval_suite(env_cfg: kcfg.EnvConfig, *, seed: int = 700001, stage_index: int = 0, n_episodes: int = 10,
                                      device: torch.device | int = 0) -> dict[str, np.ndarray]:
    """Per episode: start = clip(start_q + U(-start_noise, start_noise)) (draws only if any noise > 0), goal likewise."""
    c = env_cfg.c
    if not c.curriculum_enabled:
        raise ValueError("Curriculum-local eval requires curriculum to be enabled")
    if c.n_stages <= 0:
        raise ValueError("No curriculum stages are defined")
    idx = int(np.clip(stage_index, 0, c.n_stages - 1))
    st = c.stages[idx]
    lo, hi = np.array(c.joints.lower[:]), np.array(c.joints.upper[:])
    rng = np.random.default_rng(seed)

    def sample(base, noise):
        base = np.asarray(base, dtype=float)
        noise = np.asarray(noise, dtype=float)
        if np.any(noise > 0.0):
            base = base + rng.uniform(low=-noise, high=noise)
        return np.clip(base, lo, hi)

    init = np.empty((n_episodes, 7))
    goal = np.empty((n_episodes, 7))
    for e in range(n_episodes):
        init[e] = sample(st.start_q[:], st.start_noise[:])
        goal[e] = sample(st.goal_q[:], st.goal_noise[:])
    dev = torch.device("cuda", device) if isinstance(device, int) else device
    goal_pose6 = fk_pose6(torch.tensor(goal, dtype=torch.float64, device=dev)).cpu().numpy()
    return {"initial_q": init, "goal_q": goal, "goal_pose6": goal_pose6, "stage_index": np.full(n_episodes, idx)}


# ----------------------------------------------------------------------------- readiness predicates
def _ready(pos, ori, action_norm, dq_norm, pos_thr, ori_thr, act_thr, dq_thr):
    if not (pos_thr > 0.0 and ori_thr > 0.0):
        return torch.zeros_like(pos, dtype=torch.bool)
    ok = (pos <= pos_thr) & (ori <= ori_thr)
    if act_thr > 0.0:
        ok &= action_norm <= act_thr
    if dq_thr > 0.0:
        ok &= dq_norm <= dq_thr
    return ok


def dock_coarse_ready(pos, ori, action_norm, dq_norm, r) -> torch.Tensor:
    return _ready(pos, ori, action_norm, dq_norm, r.dock_coarse_ready_pos_threshold_m, r.dock_coarse_ready_ori_threshold_rad,
                  r.dock_coarse_ready_action_threshold, r.dock_coarse_ready_dq_threshold)


def finisher_ready(pos, ori, action_norm, dq_norm, r) -> torch.Tensor:
    return _ready(pos, ori, action_norm, dq_norm, r.finisher_ready_pos_threshold_m, r.finisher_ready_ori_threshold_rad,
                  r.finisher_ready_action_threshold, r.finisher_ready_dq_threshold)


# ----------------------------------------------------------------------------- batched episode runners
def _snapshot(env: ArmKinematicVecEnv) -> dict[str, torch.Tensor]:
    info = env.info()
    return {k: info[k].t().clone().double() for k in ("q", "dq", "prev_action", "goal_q", "goal_pose6")}


_STATE_SLICES = (("q", 0, 7), ("dq", 7, 14), ("prev_action", 14, 21), ("goal_q", 21, 28), ("goal_pose6", 28, 34))
_ALIVE_CHECK_EVERY = 8      # env steps between two reads of the device's alive-episode counter


class EpisodeBuffers:
    """The per-episode accumulators of the batched evaluator (include/kp1.h kp1_eval_buffers) over ``n_episodes`` episodes: the tensors as
    attributes named after the fields of native.EvalBuffers, ``struct`` the native.EvalBuffers over them (the object keeps the tensors alive
    as long as the struct), and ``results()`` the meaning of every plane row.  The four ``hand_*`` tensors are None (NULL in the struct)
    without ``want_hand``.  Nothing here calls the library, so it works on a CPU device too (tests/test_eval_buffers_cpu.py)."""
    NAMES = tuple(name for name, _ in native.EvalBuffers._fields_)

    def __init__(self, n_episodes: int, device: torch.device, want_hand: bool) -> None:
        n, f64, i32, u8 = int(n_episodes), torch.float64, torch.int32, torch.uint8
        layout = {"metrics": ((8, n), f64), "counters": ((4, n), i32), "flags": ((4, n), u8), "state": ((n, 34), f64),
                  "hand_metrics": ((8, n), f64), "hand_step": ((n,), i32), "hand_success": ((n,), u8), "hand_state": ((n, 34), f64),
                  "n_alive": ((1,), i32)}
        self.want_hand = bool(want_hand)
        for name in self.NAMES:
            shape, dtype = layout[name]
            if name.startswith("hand_") and not self.want_hand:
                setattr(self, name, None)
            else:       # the kernels write every element of an active episode; only the alive counter is read before it is written
                setattr(self, name, (torch.zeros if name == "n_alive" else torch.empty)(shape, dtype=dtype, device=device))
        self.struct = native.EvalBuffers(*[native.ptr(getattr(self, name)) for name in self.NAMES])

    @staticmethod
    def thresholds(ready_cfg):
        """the four dock_coarse_ready thresholds (pos, ori, action, dq) as the library takes them; None without a ready config"""
        if ready_cfg is None:
            return None
        return (C.c_double * 4)(ready_cfg.dock_coarse_ready_pos_threshold_m, ready_cfg.dock_coarse_ready_ori_threshold_rad,
                                ready_cfg.dock_coarse_ready_action_threshold, ready_cfg.dock_coarse_ready_dq_threshold)

    def results(self) -> tuple[dict[str, torch.Tensor], dict[str, torch.Tensor] | None]:
        """(final_result, handoff_result) of run_episodes: which row of which plane is which key; handoff_result None without handoff buffers"""
        metrics, counters, flags = self.metrics, self.counters, self.flags
        res = {
            "success": flags[1].bool(), "final_position_error": metrics[0], "final_orientation_error": metrics[1], "min_position_error": metrics[2],
            "min_orientation_error": metrics[3], "final_action_magnitude": metrics[4], "final_dq_norm": metrics[5], "sum_action": metrics[6],
            "sum_dq": metrics[7], "ready_hit": flags[2].bool(), "max_ready_streak": counters[1], "first_ready_step": counters[2], "step_count": counters[0],
        }
        steps = res["step_count"].clamp_min(1).double()
        res["mean_action_magnitude"] = res["sum_action"] / steps
        res["mean_dq_norm"] = res["sum_dq"] / steps
        for k, lo, hi in _STATE_SLICES:
            res["state_" + k] = self.state[:, lo:hi].contiguous()
        if not self.want_hand:
            return res, None
        hand_metrics = self.hand_metrics
        hand = {"valid": flags[3].bool(), "final_position_error": hand_metrics[0], "final_orientation_error": hand_metrics[1],
                "final_action_magnitude": hand_metrics[2], "final_dq_norm": hand_metrics[3], "min_position_error": hand_metrics[4],
                "min_orientation_error": hand_metrics[5], "step_count": self.hand_step, "success": self.hand_success.bool()}
        hsteps = self.hand_step.clamp_min(1).double()
        hand["mean_action_magnitude"] = hand_metrics[6] / hsteps
        hand["mean_dq_norm"] = hand_metrics[7] / hsteps
        for k, lo, hi in _STATE_SLICES:
            hand["state_" + k] = self.hand_state[:, lo:hi].contiguous()
        return res, hand


def _start_episodes(L, env: ArmKinematicVecEnv, ready_cfg, handoff_confirm_steps: int | None, active: torch.Tensor | None, stream):
    """what both runners do between the reset and their loop: the buffers of ``env``'s episodes (handoff buffers when there are a confirm count
    and a ready config), and kp1_eval_accumulate's step 0 under the ``active`` mask on ``stream`` -> (bufs, thr, confirm)"""
    bufs = EpisodeBuffers(env.n_envs, env.device, want_hand=handoff_confirm_steps is not None and ready_cfg is not None)
    thr = bufs.thresholds(ready_cfg)
    confirm = int(handoff_confirm_steps or 0)
    bufs.active = None if active is None else active.to(env.device).to(torch.uint8).contiguous()    # lives as long as the buffers: the launch reads it
    native.check(L.kp1_eval_accumulate(env._handle, C.byref(bufs.struct), None, None, native.ptr(bufs.active), 0, thr, confirm, stream))
    return bufs, thr, confirm


def run_episodes(env: ArmKinematicVecEnv, policy: PolicyFn, reset_options: dict[str, Any], *, ready_cfg=None, handoff_confirm_steps: int | None = None,
                 active: torch.Tensor | None = None, max_steps: int | None = None) -> tuple[dict[str, torch.Tensor], dict[str, torch.Tensor] | None]:
    """All episodes in lock step until each has terminated or truncated (_run_policy / _run_approach_with_handoff).

    Returns (final_result, handoff_result): tensors over episodes.  ``handoff_confirm_steps=None`` is the reference's _run_policy (no
    handoff bookkeeping, handoff_result None); an integer is _run_approach_with_handoff: handoff_result is the snapshot at the first
    step where ``ready_streak >= handoff_confirm_steps`` (eval_pipeline_ablation.py:103 -- so 0 or less hands over at step 1), with
    ``valid`` marking who has one, and carries the action / dq means up to that step like the reference's dict.

    Per env step: the policy, the norm of its action, kp1_step, and ONE kp1_eval_accumulate launch that does the whole per-episode
    bookkeeping on the device (finals / minima / sums, success, state snapshot, ready streak, first-confirmed handoff snapshot, alive
    mask); the host looks at the alive-episode counter every _ALIVE_CHECK_EVERY steps.  Results are bit-identical to the tensor-expression
    form (_run_episodes_reference; tests/test_eval_checkpoint_gpu.py)."""
    if not isinstance(env, ArmKinematicVecEnv):
        raise TypeError("run_episodes drives an ArmKinematicVecEnv (kp1_eval_accumulate reads its handle); the route wrappers have their own evaluator")
    L = native.load()
    env.use_current_stream()
    obs = env.reset(options=reset_options).clone()
    bufs, thr, confirm = _start_episodes(L, env, ready_cfg, handoff_confirm_steps, active, None)
    limit = int(max_steps or (env.config.c.termination.max_episode_steps + 1))
    for step in range(1, limit + 1):
        if (step - 1) % _ALIVE_CHECK_EVERY == 0 and int(bufs.n_alive.item()) == 0:
            break
        action = policy(obs)
        a_norm = torch.linalg.vector_norm(action.double(), dim=1).contiguous()
        obs, _, done = env.step(action, auto_reset=False)
        obs = obs.clone()
        native.check(L.kp1_eval_accumulate(env._handle, C.byref(bufs.struct), native.ptr(a_norm), native.ptr(done), None, step, thr, confirm, None))
    return bufs.results()


def _run_episodes_reference(env: ArmKinematicVecEnv, policy: PolicyFn, reset_options: dict[str, Any], *, ready_cfg=None, handoff_confirm_steps: int | None = None,
                 active: torch.Tensor | None = None, max_steps: int | None = None) -> tuple[dict[str, torch.Tensor], dict[str, torch.Tensor] | None]:
    """The per-step bookkeeping as tensor expressions (about 45 launches and two host synchronisations per env step): the form
    run_episodes had before kp1_eval_accumulate, kept as the test reference the device kernel is compared with bit for bit.

    All episodes in lock step until each has terminated or truncated (_run_policy / _run_approach_with_handoff).

    Returns (final_result, handoff_result) as run_episodes does."""
    E = env.n_envs
    dev = env.device
    obs = env.reset(options=reset_options).clone()
    info = env.info()
    f64 = torch.float64
    alive = torch.ones(E, dtype=torch.bool, device=dev) if active is None else active.clone().to(dev)
    pos0 = info["position_error_norm"].double().clone()
    ori0 = info["orientation_error_norm"].double().clone()
    res = {
        "success": torch.zeros(E, dtype=torch.bool, device=dev), "final_position_error": pos0.clone(), "final_orientation_error": ori0.clone(),
        "min_position_error": pos0.clone(), "min_orientation_error": ori0.clone(),
        "final_action_magnitude": torch.zeros(E, dtype=f64, device=dev), "final_dq_norm": torch.zeros(E, dtype=f64, device=dev),
        "sum_action": torch.zeros(E, dtype=f64, device=dev), "sum_dq": torch.zeros(E, dtype=f64, device=dev),
        "ready_hit": torch.zeros(E, dtype=torch.bool, device=dev), "max_ready_streak": torch.zeros(E, dtype=torch.int32, device=dev),
        "first_ready_step": torch.full((E,), -1, dtype=torch.int32, device=dev), "step_count": torch.zeros(E, dtype=torch.int32, device=dev),
    }
    streak = torch.zeros(E, dtype=torch.int32, device=dev)
    state = _snapshot(env)
    hand = None
    if handoff_confirm_steps is not None and ready_cfg is not None:
        hand = {"valid": torch.zeros(E, dtype=torch.bool, device=dev)}
        hsum = {"a": torch.zeros(E, dtype=f64, device=dev), "d": torch.zeros(E, dtype=f64, device=dev)}
    limit = int(max_steps or (env.config.c.termination.max_episode_steps + 1))
    for step in range(1, limit + 1):
        if not bool(alive.any()):
            break
        action = policy(obs)
        a_norm = torch.linalg.vector_norm(action.double(), dim=1)
        obs, _, done = env.step(action, auto_reset=False)
        obs = obs.clone()
        info = env.info()
        pos = info["position_error_norm"].double()
        ori = info["orientation_error_norm"].double()
        dqn = info["executed_delta_q_l2"].double()
        upd = alive
        res["step_count"] = torch.where(upd, torch.full_like(res["step_count"], step), res["step_count"])
        res["sum_action"] += torch.where(upd, a_norm, torch.zeros_like(a_norm))
        res["sum_dq"] += torch.where(upd, dqn, torch.zeros_like(dqn))
        for key, val in (("final_position_error", pos), ("final_orientation_error", ori), ("final_action_magnitude", a_norm), ("final_dq_norm", dqn)):
            res[key] = torch.where(upd, val, res[key])
        res["min_position_error"] = torch.where(upd, torch.minimum(res["min_position_error"], pos), res["min_position_error"])
        res["min_orientation_error"] = torch.where(upd, torch.minimum(res["min_orientation_error"], ori), res["min_orientation_error"])
        res["success"] = torch.where(upd, (done & 4) != 0, res["success"])
        snap = _snapshot(env)
        for k in state:
            state[k] = torch.where(upd[:, None], snap[k], state[k])
        if ready_cfg is not None:
            rdy = dock_coarse_ready(pos, ori, a_norm, dqn, ready_cfg) & upd
            res["ready_hit"] |= rdy
            res["first_ready_step"] = torch.where(rdy & (res["first_ready_step"] < 0), torch.full_like(res["first_ready_step"], step), res["first_ready_step"])
            streak = torch.where(upd, torch.where(rdy, streak + 1, torch.zeros_like(streak)), streak)
            res["max_ready_streak"] = torch.maximum(res["max_ready_streak"], streak)
            if hand is not None:
                take = upd & (~hand["valid"]) & (streak >= handoff_confirm_steps)
                hsum["a"] = torch.where(take, res["sum_action"], hsum["a"])
                hsum["d"] = torch.where(take, res["sum_dq"], hsum["d"])
                if bool(take.any()):
                    cur = {"final_position_error": pos, "final_orientation_error": ori, "final_action_magnitude": a_norm, "final_dq_norm": dqn,
                           "min_position_error": res["min_position_error"], "min_orientation_error": res["min_orientation_error"],
                           "step_count": torch.full_like(res["step_count"], step), "success": (done & 4) != 0, **{"state_" + k: v for k, v in snap.items()}}
                    for k, v in cur.items():
                        if k not in hand:
                            hand[k] = torch.zeros_like(v)
                        m = take if v.ndim == 1 else take[:, None]
                        hand[k] = torch.where(m, v, hand[k])
                    hand["valid"] |= take
        alive = alive & ((done & 3) == 0)
    steps = res["step_count"].clamp_min(1).double()
    res["mean_action_magnitude"] = res["sum_action"] / steps
    res["mean_dq_norm"] = res["sum_dq"] / steps
    for k, v in state.items():
        res["state_" + k] = v
    if hand is not None and "step_count" in hand:
        hsteps = hand["step_count"].clamp_min(1).double()
        hand["mean_action_magnitude"] = hsum["a"] / hsteps
        hand["mean_dq_norm"] = hsum["d"] / hsteps
    return res, hand


def _is_fused_width(mlp: Any) -> bool:
    """an MlpKernels the one-launch evaluation step covers, on the 56-float observation: the layer-wise widths (K = 1 or a population), or a
    K = 1 handle of hidden 256 whose tile path is on (kp1_eval_step refuses a 2x256 handle switched to the layer-wise kernels)"""
    if mlp is None or int(getattr(mlp, "obs_dim", 0)) != kcfg.OBS_DIM:
        return False
    hidden = int(getattr(mlp, "hidden", 0))
    if hidden == 256:
        return int(getattr(mlp, "replicas", 1)) == 1 and bool(getattr(mlp, "fused", True))
    return hidden in (64, 128)


def policy_mlp(policy: Any) -> Any:
    """the MlpKernels behind a policy callable, or None: an InferencePolicy or a PPO exposes it as ``_mlp``, a bound ``predict`` method of one
    through ``__self__``; any other callable (a function, a lambda, a wrapper around predict) is not looked into"""
    owner = getattr(policy, "__self__", None)
    if owner is None:
        return getattr(policy, "_mlp", None)
    return getattr(owner, "_mlp", None) if getattr(policy, "__name__", "") == "predict" else None


def _one_launch_mlp(policy: Any, env: Any, one_launch: bool | None, what: str) -> Any:
    """the handle run_episodes_fused steps ``env`` with, or None for run_episodes.  ``one_launch``: None = the one-launch step where it is
    covered (a K = 1 handle _is_fused_width accepts behind ``policy``, an fp32 ArmKinematicVecEnv), False = never, True = ValueError when not"""
    if one_launch is False:
        return None
    mlp = policy_mlp(policy)
    covered = (_is_fused_width(mlp) and int(getattr(mlp, "replicas", 1)) == 1 and isinstance(env, ArmKinematicVecEnv)
               and env.dtype == torch.float32)
    if covered:
        return mlp
    if one_launch:
        raise ValueError(f"one_launch=True: the {what} phase is not covered by the one-launch evaluation step (it takes a policy backed by a "
                         "K = 1 MlpKernels of hidden 64 / 128 / 256 on the 56-float observation, tile path on for 256, and an fp32 "
                         "ArmKinematicVecEnv)")
    return None


# Which entry points run their covered phases through kp1_eval_episodes (all env steps of a phase in one launch) when their
# ``whole_episodes`` keyword is None.  Set by the acceptance rule of DESIGN section 20 applied to tools/eval_episode_bench.py
# (profiles/eval_episodes.json): True only where the whole-episode median beats the per-step median by more than the
# per-step form's own max - min spread; an entry point that was not measured stays False.
WHOLE_EPISODES_DEFAULT: dict[str, bool] = {
    "evaluate_workspace_expansion": False,               # gate evaluation: 9.46 -> 9.03 ms (spread 0.19) at confirm 2, but 11.14 -> 11.25 (3.01) at confirm 0
    "run_pairs": False,                                  # 8192 pairs: 8.45 -> 7.35 ms, inside the per-step form's spread of 1.48 ms
    "evaluate_workspace_expansion_population": False,    # not measured
    "evaluate_dock": True,                               # 512 episodes: 1.60 -> 1.54 ms (spread 0.05)
}
# env steps of one kp1_eval_episodes call (a longer limit is split into consecutive calls)
_EPISODES_CAP = native.EVAL_EPISODES_MAX_STEPS


def whole_episodes_default(entry: str, whole_episodes: bool | None) -> bool:
    """an entry point's ``whole_episodes`` keyword resolved: None is the entry point's row of WHOLE_EPISODES_DEFAULT"""
    return WHOLE_EPISODES_DEFAULT[entry] if whole_episodes is None else bool(whole_episodes)


def _uncovered_whole_episodes(what: str) -> ValueError:
    return ValueError(f"whole_episodes=True: the {what} phase is not covered by the whole-episode evaluation kernel (it covers what the one-launch "
                      "evaluation step covers, and one_launch must not be False)")


def run_phase(env: ArmKinematicVecEnv, policy: Any, reset_options: dict[str, Any], *, one_launch: bool | None, what: str,
              whole_episodes: bool | None = None, entry: str | None = None, **kw):
    """one evaluation phase through run_episodes_fused when ``one_launch`` allows it and the phase is covered, else through run_episodes.
    ``whole_episodes`` (None: the default of ``entry``, False without one) picks kp1_eval_episodes for a covered phase; True on a phase
    that is not covered raises ValueError, as ``one_launch=True`` does."""
    mlp = _one_launch_mlp(policy, env, one_launch, what)
    if mlp is not None:
        whole = bool(whole_episodes) if (whole_episodes is not None or entry is None) else WHOLE_EPISODES_DEFAULT[entry]
        return run_episodes_fused(env, mlp, reset_options, whole_episodes=whole, **kw)
    if whole_episodes:
        raise _uncovered_whole_episodes(what)
    return run_episodes(env, policy, reset_options, **kw)


def run_episodes_fused(env: ArmKinematicVecEnv, mlp: Any, reset_options: dict[str, Any], *, ready_cfg=None, handoff_confirm_steps: int | None = None,
                       active: torch.Tensor | None = None, max_steps: int | None = None,
                       whole_episodes: bool = False) -> tuple[dict[str, torch.Tensor], dict[str, torch.Tensor] | None]:
    """run_episodes with the whole env step in ONE launch (kp1_eval_step): the deterministic policy of ``mlp`` (an MlpKernels of hidden 64 /
    128: a K = 1 handle, or a population handle of K replicas over ``env``'s K x n envs, block k of the envs stepping under replica k's
    weights; or a K = 1 handle of hidden 256 with the tile path on, a training handle included: the step reads its packed weights and
    touches no workspace), the fp64 norm of the clipped action, the env step and the per-episode bookkeeping.  The observations stay in the env's own
    buffer, which the launch reads and overwrites.  Same return value as run_episodes; every tensor not derived from the action norm is
    bit-equal to it, and the action-norm tensors are the norm summed in index order (tests/test_population_eval_gpu.py,
    tests/test_eval_step_h256_gpu.py).

    ``whole_episodes=True`` replaces the per-step loop and its counter read-backs by kp1_eval_episodes: all env steps in one launch per
    256 steps of the limit (a later call is skipped once no episode is alive).  Every returned tensor is bit-equal to the per-step form's
    (tests/test_eval_episodes_gpu.py); the env handle is left with every episode at its own last step instead of stepped on in lock step."""
    if not isinstance(env, ArmKinematicVecEnv):
        raise TypeError("run_episodes_fused drives an ArmKinematicVecEnv (kp1_eval_step steps its handle)")
    L = native.load()
    env.use_current_stream()
    stream = native.stream_arg(env.device)
    env.reset(options=reset_options)
    bufs, thr, confirm = _start_episodes(L, env, ready_cfg, handoff_confirm_steps, active, stream)
    limit = int(max_steps or (env.config.c.termination.max_episode_steps + 1))
    if whole_episodes:
        for first in range(1, limit + 1, _EPISODES_CAP):
            if first > 1 and int(bufs.n_alive.item()) == 0:
                break
            native.check(L.kp1_eval_episodes(mlp._h, env._handle, native.ptr(env.obs), native.ptr(env.reward), native.ptr(env.done), C.byref(bufs.struct), first,
                                             min(first + _EPISODES_CAP - 1, limit), thr, confirm, stream))
    else:
        for step in range(1, limit + 1):
            if (step - 1) % _ALIVE_CHECK_EVERY == 0 and int(bufs.n_alive.item()) == 0:
                break
            native.check(L.kp1_eval_step(mlp._h, env._handle, native.ptr(env.obs), native.ptr(env.reward), native.ptr(env.done), C.byref(bufs.struct), step, thr, confirm,
                                         stream))
    return bufs.results()


def _handoff_options(src: dict[str, torch.Tensor], mode: str) -> dict[str, Any]:
    """_state_reset_options; eval_three_stage.py:30-38"""
    return {"initial_q": src["state_q"].cpu().numpy(), "initial_dq": src["state_dq"].cpu().numpy(),
            "initial_prev_action": src["state_prev_action"].cpu().numpy(), "goal_q": src["state_goal_q"].cpu().numpy(),
            "goal_pose6": src["state_goal_pose6"].cpu().numpy(), "policy_mode": mode}


def _mean(x) -> float:
    x = np.asarray(x, dtype=float)
    return float(x.mean()) if x.size else 0.0


def evaluate_workspace_expansion(*, approach_policy: PolicyFn, finisher_policy: PolicyFn | None, approach_cfg: kcfg.EnvConfig,
                                 finisher_cfg: kcfg.EnvConfig | None, episodes: int = 50, seed: int = 700001,
                                 stage_indices: list[int] | None = None, handoff_confirm_steps: int = 2, gate_config: dict[str, Any] | None = None,
                                 artifact_root: str | Path | None = None, device: int = 0, obs_stride: int = 56,
                                 one_launch: bool | None = None, whole_episodes: bool | None = None) -> dict[str, Any]:
    """evaluate_workspace_expansion_checkpoint with policies passed as callables (checkpoint loading is the caller's).

    ``whole_episodes``: None (default) is this entry point's row of WHOLE_EPISODES_DEFAULT; True runs every phase through kp1_eval_episodes
    (all env steps of the phase in one launch, same payload bit for bit) and raises ValueError for a phase that is not covered; False keeps
    one launch per env step.

    ``one_launch``: None (default) runs a phase through run_episodes_fused -- one launch per env step -- when its policy is an InferencePolicy /
    PPO (or a bound ``predict`` of one) on a handle the step covers, and through run_episodes otherwise; False always takes run_episodes; True
    raises ValueError for a phase that is not covered.  The two forms agree bit for bit except in the action-magnitude floats, which may
    differ by an ulp (the norm is summed in index order instead of vector_norm's reduction)."""
    stages, cat = _stage_suite(approach_cfg, seed, stage_indices, episodes, device)
    E = cat["initial_q"].shape[0]
    r = approach_cfg.c.reward
    env_kw = dict(device=device, seed=seed, obs_stride=obs_stride)
    phase = dict(one_launch=one_launch, whole_episodes=whole_episodes, entry="evaluate_workspace_expansion")

    env = _phase_env(approach_cfg, E, **env_kw)
    a_res, hand = run_phase(env, approach_policy, {"initial_q": cat["initial_q"], "goal_q": cat["goal_q"], "goal_pose6": cat["goal_pose6"],
                                                   "policy_mode": "approach"}, what="Approach", ready_cfg=r,
                            handoff_confirm_steps=handoff_confirm_steps, **phase)
    env.close()
    final_ready, has_hand, f_res = _finisher_phase(a_res, hand, r, finisher_policy, finisher_cfg, env_kw, **phase)
    cols = _eval_columns(a_res, final_ready, has_hand, f_res, handoff_confirm_steps)
    return _workspace_payload(cols, cat["goal_pose6"], approach_cfg=approach_cfg, stages=stages, episodes=episodes, seed=seed,
                              handoff_confirm_steps=handoff_confirm_steps, gate_config=gate_config, artifact_root=artifact_root)


def _stage_suite(approach_cfg: kcfg.EnvConfig, seed: int, stage_indices: list[int] | None, episodes: int, device) -> tuple[list[int], dict[str, np.ndarray]]:
    """(stages, cat): the stage list clipped to the curriculum (every stage when none is given) and the curriculum-local suites of those
    stages, ``episodes`` each, concatenated in that order"""
    n_stages = approach_cfg.n_stages
    stages = stage_indices if stage_indices is not None else list(range(n_stages))
    stages = [int(np.clip(s, 0, n_stages - 1)) for s in stages]
    suites = [build_curriculum_local_eval_suite(approach_cfg, seed=seed + s * 1009, stage_index=s, n_episodes=episodes, device=device) for s in stages]
    return stages, {k: np.concatenate([su[k] for su in suites]) for k in suites[0]}


def _phase_env(cfg: kcfg.EnvConfig, n: int, *, device, seed: int, obs_stride: int, first_env_id: int = 0) -> ArmKinematicVecEnv:
    """the env of one evaluation phase: n envs of ``cfg`` (env k is global env first_env_id + k) at the policy's observation row pitch"""
    env = ArmKinematicVecEnv(cfg, n, device=device, seed=seed, first_env_id=first_env_id)
    if obs_stride != 56:
        env.set_obs_stride(obs_stride)
    return env


def _finisher_phase(a_res: dict[str, torch.Tensor], hand: dict[str, torch.Tensor], r, finisher_policy: Any, finisher_cfg: kcfg.EnvConfig | None,
                    env_kw: dict[str, Any], **phase) -> tuple[torch.Tensor, torch.Tensor, dict[str, torch.Tensor] | None]:
    """the second half of a two-phase run, from the Approach results -> (final_ready, has_hand, f_res).  Where there are a Finisher policy and
    config and any row hands over, a Finisher env like the Approach one (``env_kw``: _phase_env's keywords) is reset to the handoff sources
    and run under ``active=has_hand`` by run_phase (``phase``: its one_launch / whole_episodes / entry); f_res is None otherwise."""
    final_ready, has_hand, src = _handoff_sources(a_res, hand, r)
    f_res = None
    if finisher_policy is not None and finisher_cfg is not None and bool(has_hand.any()):
        fenv = _phase_env(finisher_cfg, has_hand.shape[0], **env_kw)
        # rows without a handoff still need finite reset inputs; they are masked out of every result
        safe = {k: torch.where(has_hand[:, None], v, a_res[k]) for k, v in src.items()}
        f_res, _ = run_phase(fenv, finisher_policy, _handoff_options(safe, "dock"), what="Finisher", active=has_hand, **phase)
        fenv.close()
    return final_ready, has_hand, f_res


def _merge_finisher(a_res: dict[str, torch.Tensor], has_hand: torch.Tensor, f_res: dict[str, torch.Tensor] | None) -> tuple[dict[str, torch.Tensor], torch.Tensor]:
    """(final, success) of a two-phase run: the Approach's four finals and success, replaced by the Finisher's in the rows that were handed over"""
    final = {k: a_res[k].clone() for k in ("final_position_error", "final_orientation_error", "final_action_magnitude", "final_dq_norm")}
    success = a_res["success"].clone()
    if f_res is not None:
        for k in final:
            final[k] = torch.where(has_hand, f_res[k], final[k])
        success = torch.where(has_hand, f_res["success"], success)
    return final, success


def _handoff_sources(a_res: dict[str, torch.Tensor], hand: dict[str, torch.Tensor], r) -> tuple[torch.Tensor, torch.Tensor, dict[str, torch.Tensor]]:
    """(final_ready, has_hand, src) of an Approach phase: the handoff source of a row is its final state if that is finisher-ready, else the
    first confirmed-ready snapshot (eval_workspace_expansion.py:138-139)"""
    final_ready = finisher_ready(a_res["final_position_error"], a_res["final_orientation_error"], a_res["final_action_magnitude"], a_res["final_dq_norm"], r)
    has_hand = final_ready | hand["valid"]
    src = {}
    for k in ("state_q", "state_dq", "state_prev_action", "state_goal_q", "state_goal_pose6"):
        hk = hand.get(k, torch.zeros_like(a_res[k]))
        src[k] = torch.where(final_ready[:, None], a_res[k], hk)
    return final_ready, has_hand, src


def _eval_columns(a_res: dict[str, torch.Tensor], final_ready: torch.Tensor, has_hand: torch.Tensor, f_res: dict[str, torch.Tensor] | None,
                  handoff_confirm_steps: int, rows: slice = slice(None)) -> dict[str, Any]:
    """the per-episode host columns the row / summary code reads, for episodes ``rows`` of the run (a replica's block of a population run):
    the Approach results (A), the finals after the Finisher where one ran (F), success, ready hit / dwell and the two regression flags"""
    final, success = _merge_finisher(a_res, has_hand, f_res)
    ready_hit = a_res["ready_hit"] | final_ready
    ready_dwell = (a_res["max_ready_streak"] >= handoff_confirm_steps) | final_ready
    pos_reg = a_res["final_position_error"] > a_res["min_position_error"] + 0.002
    ori_reg = a_res["final_orientation_error"] > a_res["min_orientation_error"] + 0.01

    def cpu(t):
        return t[rows].detach().cpu().numpy()

    return {"A": {k: cpu(v) for k, v in a_res.items() if v.ndim == 1}, "F": {k: cpu(v) for k, v in final.items()}, "success": cpu(success),
            "ready_hit": cpu(ready_hit), "ready_dwell": cpu(ready_dwell), "position_regression": cpu(pos_reg), "orientation_regression": cpu(ori_reg)}


def _workspace_payload(cols: dict[str, Any], goal_pose6: np.ndarray, *, approach_cfg: kcfg.EnvConfig, stages: list[int], episodes: int, seed: int,
                       handoff_confirm_steps: int, gate_config: dict[str, Any] | None, artifact_root: str | Path | None) -> dict[str, Any]:
    """target rows, per-stage summaries and the gated selection of one policy's evaluation from its host columns (_eval_columns; episode
    e of stage number si is column si * episodes + e), written under ``artifact_root`` when one is given"""
    r = approach_cfg.c.reward
    A, F = cols["A"], cols["F"]
    succ, rh, rd, pr, orr = cols["success"], cols["ready_hit"], cols["ready_dwell"], cols["position_regression"], cols["orientation_regression"]
    cat = {"goal_pose6": goal_pose6}
    rows: list[dict[str, Any]] = []
    stage_summaries: dict[int, dict[str, Any]] = {}
    for si, s in enumerate(stages):
        sl = slice(si * episodes, (si + 1) * episodes)
        metrics = []
        for e in range(sl.start, sl.stop):
            if succ[e]:
                reason = "success"
            elif A["final_position_error"][e] > r.finisher_ready_pos_threshold_m:
                reason = "position"
            elif A["final_orientation_error"][e] > r.finisher_ready_ori_threshold_rad:
                reason = "orientation"
            elif A["final_action_magnitude"][e] > r.finisher_ready_action_threshold:
                reason = "motion_action"
            elif A["final_dq_norm"][e] > r.finisher_ready_dq_threshold:
                reason = "motion_dq"
            elif not bool(A["max_ready_streak"][e] >= handoff_confirm_steps):
                reason = "dwell"
            else:
                reason = "timeout_or_regression"
            metrics.append({
                "episode_id": e - sl.start, "stage_index": int(s), "stage_name": approach_cfg.stage_names[s] if approach_cfg.stage_names else str(s),
                "success": bool(succ[e]), "finisher_ready_hit": bool(rh[e]), "finisher_ready_dwell": bool(rd[e]), "failure_reason": reason,
                "final_position_error": float(F["final_position_error"][e]), "final_orientation_error": float(F["final_orientation_error"][e]),
                "approach_final_position_error": float(A["final_position_error"][e]), "approach_final_orientation_error": float(A["final_orientation_error"][e]),
                "final_action_magnitude": float(F["final_action_magnitude"][e]), "final_dq_norm": float(F["final_dq_norm"][e]),
                "min_position_error": float(A["min_position_error"][e]), "min_orientation_error": float(A["min_orientation_error"][e]),
                "position_regression": bool(pr[e]), "orientation_regression": bool(orr[e]),
                "goal_position": cat["goal_pose6"][e][:3].tolist(), "goal_orientation": cat["goal_pose6"][e][3:].tolist(),
            })
        reasons: dict[str, int] = {}
        for mrow in metrics:
            reasons[mrow["failure_reason"]] = reasons.get(mrow["failure_reason"], 0) + 1
        stage_summaries[s] = {
            "episode_count": len(metrics), "success_rate": _mean([m["success"] for m in metrics]),
            "finisher_ready_hit_rate": _mean([m["finisher_ready_hit"] for m in metrics]), "dwell_success_rate": _mean([m["finisher_ready_dwell"] for m in metrics]),
            "mean_final_position_error": _mean([m["final_position_error"] for m in metrics]),
            "mean_final_orientation_error": _mean([m["final_orientation_error"] for m in metrics]),
            "mean_final_action_magnitude": _mean([m["final_action_magnitude"] for m in metrics]), "mean_final_dq_norm": _mean([m["final_dq_norm"] for m in metrics]),
            "regression_rate": _mean([m["position_regression"] or m["orientation_regression"] for m in metrics]), "failure_reason_counts": reasons,
        }
        rows.extend(metrics)
    gcfg = gate_config_from_dict(gate_config)
    score_stage = int(np.clip(int((gate_config or {}).get("score_stage_index", max(stages))), min(stages), max(stages)))
    selection = gated_score(stage_summaries, score_stage, gcfg)
    payload = {"episodes_per_stage": int(episodes), "seed": int(seed), "stage_metrics": {str(k): v for k, v in stage_summaries.items()},
               "best_model_selection": selection, "target_rows": rows}
    if artifact_root is not None:
        root = Path(artifact_root)
        root.mkdir(parents=True, exist_ok=True)
        (root / "stage_metrics.json").write_text(json.dumps(payload["stage_metrics"], indent=2))
        (root / "best_model_selection_summary.json").write_text(json.dumps(selection, indent=2))
        (root / "workspace_eval_summary.json").write_text(json.dumps(payload, indent=2))
    return payload


def check_population_eval(population: Any, artifact_roots: list[Any] | None) -> int:
    """the host-side refusals of evaluate_workspace_expansion_population, before any device call; returns K"""
    K = int(population.K)
    if artifact_roots is not None and len(artifact_roots) != K:
        raise ValueError(f"{len(artifact_roots)} artifact roots for a population of {K} replicas: the evaluator writes one set of files per replica")
    if int(getattr(population, "obs_dim", kcfg.OBS_DIM)) != kcfg.OBS_DIM:
        raise ValueError("evaluate_workspace_expansion_population evaluates Approach populations (56-float observation); a route population has "
                         "its own evaluator")
    hidden = int(population.cfg.hidden)
    if hidden not in (64, 128):
        raise ValueError(f"evaluate_workspace_expansion_population runs the one-launch evaluation step of the 2x64 / 2x128 nets; hidden={hidden} "
                         "is evaluated per policy with evaluate_workspace_expansion")
    return K


def evaluate_workspace_expansion_population(*, population: Any, finisher_policy: Any, approach_cfg: kcfg.EnvConfig, finisher_cfg: kcfg.EnvConfig | None,
                                            episodes: int = 50, seed: int = 700001, stage_indices: list[int] | None = None,
                                            handoff_confirm_steps: int = 2, gate_config: dict[str, Any] | None = None,
                                            artifact_roots: list[str | Path] | None = None, device: int = 0,
                                            whole_episodes: bool | None = None) -> list[dict[str, Any]]:
    """evaluate_workspace_expansion of every replica of a PopulationPPO at once: K payloads (and K sets of JSON files under
    ``artifact_roots[k]``), each what ``evaluate_workspace_expansion(approach_policy=population.replica(k).predict, ...)`` returns up to
    the summation order of the action norm.

    The suite is built once and tiled K times into one Approach handle of K x E envs; block k steps under replica k's weights as the
    population's own training handle holds them (no parameter copy, no repack), one kp1_eval_step launch per env step for all replicas.
    The Finisher phase is one run over all K x E rows with the shared Finisher policy (``finisher_policy``: an InferencePolicy, stepped in
    one launch when kp1_eval_step covers its handle -- 64 / 128 wide, or 2x256 on the tile kernels -- and through run_episodes otherwise;
    run_phase decides, so a bound ``predict`` of one is looked through as in evaluate_workspace_expansion).
    Episodes of different replicas run in lock step until none of any replica is alive; a finished episode's bookkeeping is frozen, so the
    extra steps change nothing in its block.

    ``whole_episodes`` as in evaluate_workspace_expansion (None: this entry point's row of WHOLE_EPISODES_DEFAULT): True runs both phases
    through kp1_eval_episodes and raises ValueError when the Finisher policy's handle is not covered."""
    K = check_population_eval(population, artifact_roots)
    whole = whole_episodes_default("evaluate_workspace_expansion_population", whole_episodes)
    stages, cat = _stage_suite(approach_cfg, seed, stage_indices, episodes, device)
    E = cat["initial_q"].shape[0]
    r = approach_cfg.c.reward
    env_kw = dict(device=device, seed=seed, obs_stride=int(population.obs_w))

    env = _phase_env(approach_cfg, K * E, **env_kw)
    tiled = {k: np.tile(cat[k], (K, 1)) for k in ("initial_q", "goal_q", "goal_pose6")}
    a_res, hand = run_episodes_fused(env, population._mlp, {**tiled, "policy_mode": "approach"}, ready_cfg=r, handoff_confirm_steps=handoff_confirm_steps,
                                     whole_episodes=whole)
    env.close()
    # the shared Finisher policy picks its runner as in evaluate_workspace_expansion(one_launch=None)
    final_ready, has_hand, f_res = _finisher_phase(a_res, hand, r, finisher_policy, finisher_cfg, env_kw, one_launch=None,
                                                   whole_episodes=whole_episodes, entry="evaluate_workspace_expansion_population")
    payloads = []
    for k in range(K):
        cols = _eval_columns(a_res, final_ready, has_hand, f_res, handoff_confirm_steps, rows=slice(k * E, (k + 1) * E))
        payloads.append(_workspace_payload(cols, cat["goal_pose6"], approach_cfg=approach_cfg, stages=stages, episodes=episodes, seed=seed,
                                           handoff_confirm_steps=handoff_confirm_steps, gate_config=gate_config,
                                           artifact_root=None if artifact_roots is None else artifact_roots[k]))
    return payloads
