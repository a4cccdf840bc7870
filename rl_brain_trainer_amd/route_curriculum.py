"""Route prefix curriculum and the sequential route evaluator on the device engine.

What the reference does in kinematic_phase1/route/route_curriculum.py:17-136 (``RoutePrefixCurriculumCallback``: four sliding windows over
finished episodes, promotion to the next route prefix when all four rates pass) runs here as a one-wave device tracker
(include/kp1_route.h, kp1_route_curriculum_*) so the PPO rollout stays one hipGraph replay; this module holds its host handle.
kinematic_phase1/eval/eval_route_curriculum.py:57-248 (sequential evaluation: the final (q, dq, prev_action) of waypoint k start
waypoint k+1) and eval/eval_route_gate.py:17-99 (accept / reject of a checkpoint from per-prefix evaluations) keep their JSON schemas --
status scripts read them -- with the bookkeeping done on numeric columns.
"""
from __future__ import annotations

import ctypes as C

import json
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Callable, Sequence

import numpy as np
import torch

from . import config as kcfg
from . import native
from . import route_config as rcfg
from .curriculum import DeviceTracker, TrackerPopulation, TrackerReplica, window_mean
from .route_env import RoutePopulationVecEnv, RouteVecEnv


@dataclass(frozen=True)
class RouteCurriculumStage:
    name: str
    prefix_end_index: int


def build_prefix_stages(prefixes: Sequence[int]) -> list[RouteCurriculumStage]:
    return [RouteCurriculumStage(name=f"prefix_{int(p)}", prefix_end_index=int(p)) for p in prefixes]


# --------------------------------------------------------------------------------------------- the same callback on the device
MAX_STAGES, MAX_WINDOW, MAX_HISTORY = (native.header_int("KP1_ROUTE_CURRICULUM_MAX_" + n) for n in ("STAGES", "WINDOW", "HISTORY"))


class _CurriculumEvent(C.Structure):
    _fields_ = [("total_timesteps", C.c_int64), ("from_stage", C.c_int32), ("to_stage", C.c_int32), ("from_prefix_end_index", C.c_int32),
                ("to_prefix_end_index", C.c_int32), ("recent_success_rate", C.c_double), ("recent_route_ready_hit_rate", C.c_double),
                ("recent_orientation_hit_rate", C.c_double), ("recent_regression_rate", C.c_double)]


class _CurriculumState(C.Structure):
    _fields_ = [("stage_index", C.c_int32), ("stage_episode_count", C.c_int32), ("ring_len", C.c_int32), ("ring_head", C.c_int32),
                ("window_episodes", C.c_int32), ("min_episodes_per_stage", C.c_int32), ("n_stages", C.c_int32), ("n_events", C.c_int32),
                ("prefix_end_index", C.c_int32 * MAX_STAGES), ("ring_sums", C.c_int32 * 4), ("promotion_success_rate", C.c_double), ("promotion_route_ready_hit_rate", C.c_double),
                ("promotion_orientation_hit_rate", C.c_double), ("promotion_max_regression_rate", C.c_double), ("num_timesteps", C.c_int64),
                ("ring", (C.c_uint8 * MAX_WINDOW) * 4), ("events", _CurriculumEvent * MAX_HISTORY)]


class RoutePrefixCurriculumDevice(DeviceTracker):
    """RoutePrefixCurriculum with the per-step scan on the device (include/kp1_route.h, kp1_route_curriculum_*): same promotion rule and
    history, no host synchronisation per step, so the PPO rollout stays one hipGraph replay.  Plugs into ``PPO(curriculum=...)``.

    Data parallel: the tracker needs the wrapper's per-env flags as well as the done bytes, and the flags are overwritten by every step, so
    PPO records each step (``record``: one byte per env, done bits + flags) and exchanges those records once per chunk (``observe_chunk``)."""

    State = _CurriculumState
    needs_episode_records = True

    def __init__(self, *, stages: list[RouteCurriculumStage], promotion_success_rate: float, promotion_route_ready_hit_rate: float,
                 promotion_orientation_hit_rate: float, promotion_max_regression_rate: float, window_episodes: int, min_episodes_per_stage: int = 128) -> None:
        if not stages:
            raise ValueError("RoutePrefixCurriculumCallback requires at least one stage")
        if len(stages) > MAX_STAGES or int(window_episodes) > MAX_WINDOW:
            raise ValueError(f"the device tracker holds at most {MAX_STAGES} stages and a window of {MAX_WINDOW} episodes")
        self.stages = list(stages)
        self._args = (float(promotion_success_rate), float(promotion_route_ready_hit_rate), float(promotion_orientation_hit_rate),
                      float(promotion_max_regression_rate), max(int(window_episodes), 1), max(int(min_episodes_per_stage), 1))
        self.env: RouteVecEnv | None = None
        self._st = C.c_void_p()

    @classmethod
    def from_config(cls, cfg: dict[str, Any], n_waypoints: int) -> "RoutePrefixCurriculumDevice":
        """``route.curriculum`` block of the YAML with the trainer's defaults (train_route_curriculum.py:86-88, 150-160)"""
        block = dict((cfg.get("route", {}) or {}).get("curriculum", {}) or {})
        defaults = {"promotion_success_rate": 0.80, "promotion_route_ready_hit_rate": 0.80, "promotion_orientation_hit_rate": 0.90,
                    "promotion_max_regression_rate": 0.20}
        rates = {k: float(block.get(k, v)) for k, v in defaults.items()}
        return cls(stages=build_prefix_stages(rcfg.prefix_stages(cfg, n_waypoints)), window_episodes=int(block.get("promotion_window_episodes", 256)),
                   min_episodes_per_stage=int(block.get("min_episodes_per_stage", 128)), **rates)

    @property
    def window_episodes(self) -> int:
        return int(self._args[4])

    @property
    def min_episodes_per_stage(self) -> int:
        return int(self._args[5])

    @property
    def promotion_max_regression_rate(self) -> float:
        return float(self._args[3])

    def _create(self, env: RouteVecEnv, create: Callable[..., int]) -> tuple[int, int]:
        """attach: the tracker(s) next to the env by ``create``, and the env's reset window on the first prefix; returns that window"""
        self.env = env
        prefixes = (C.c_int32 * len(self.stages))(*[int(s.prefix_end_index) for s in self.stages])
        with torch.cuda.device(env.device):
            native.check(create(env._handle, prefixes, len(self.stages), *self._args, C.byref(self._st)))
        env.route_cfg.reset.min_route_index, env.route_cfg.reset.max_route_index = first = (1, int(prefixes[0]))
        return first

    def attach(self, env: RouteVecEnv) -> None:
        """_on_training_start: allocate the tracker next to the env and apply the first prefix."""
        self._create(env, env.L.kp1_route_curriculum_create)

    def observe(self, dones: torch.Tensor, steps_per_call: int) -> None:
        if dones.numel() != self.env.n_envs:
            raise ValueError("observe() tracks one process's envs from the env's own flags; data parallel goes through record() + observe_chunk()")
        native.check(self.env.L.kp1_route_curriculum_observe(self.env._handle, self._st, native.ptr(dones), int(steps_per_call), self._stream()))

    def record(self, dones: torch.Tensor, out: torch.Tensor) -> None:
        """out[N] <- this step's episode records: the KP1_DONE_* bits of ``dones`` | route_ready << 4 | orientation hit << 5 | regression << 6,
        the flags read from the env's planes on the device (call after the step, before the next one rewrites them)"""
        n = self.env.n_envs
        if dones.numel() != n or out.numel() != n or out.dtype != torch.uint8 or not (dones.is_contiguous() and out.is_contiguous()):
            raise ValueError(f"record() takes the {n} done bytes of one step and a contiguous uint8 [{n}] output")
        native.check(self.env.L.kp1_route_episode_records(self.env._handle, native.ptr(dones), native.ptr(out), self._stream()))

    def observe_chunk(self, records_all: torch.Tensor, n_local: int, chunk_steps: int, world: int) -> None:
        """data-parallel rollouts: the all-gathered [world, chunk_steps, n_local] episode records of a chunk of env steps, replayed in the
        reference's order (step by step, global env id order inside a step); a promotion moves this rank's reset window"""
        if not (records_all.numel() == world * chunk_steps * n_local and records_all.dtype == torch.uint8 and records_all.is_contiguous()):
            raise ValueError(f"observe_chunk() takes contiguous uint8 records of shape [{world}, {chunk_steps}, {n_local}]")
        native.check(self.env.L.kp1_route_curriculum_observe_chunk(self.env._handle, self._st, native.ptr(records_all), int(n_local),
                                                                   int(chunk_steps), int(world), self._stream()))

    def _read_call(self, k: int, out: Any, stream: C.c_void_p) -> int:
        return self.env.L.kp1_route_curriculum_read(self.env._handle, self._st, out, stream)

    def _follow(self, st: _CurriculumState, k: int) -> None:
        self.env.route_cfg.reset.min_route_index, self.env.route_cfg.reset.max_route_index = 1, int(st.prefix_end_index[st.stage_index])

    def _summary_of(self, st: _CurriculumState) -> dict[str, object]:
        history = []
        for k in range(min(int(st.n_events), MAX_HISTORY)):
            e = st.events[k]
            history.append({"from_stage": self.stages[e.from_stage].name, "to_stage": self.stages[e.to_stage].name,
                            "from_prefix_end_index": int(e.from_prefix_end_index), "to_prefix_end_index": int(e.to_prefix_end_index),
                            "total_timesteps": int(e.total_timesteps), "recent_success_rate": float(e.recent_success_rate),
                            "recent_route_ready_hit_rate": float(e.recent_route_ready_hit_rate),
                            "recent_orientation_hit_rate": float(e.recent_orientation_hit_rate), "recent_regression_rate": float(e.recent_regression_rate)})
        stage = self.stages[int(st.stage_index)]
        mean = [window_mean(st, st.ring[q]) for q in range(4)]
        return {"stage_index": int(st.stage_index), "stage_name": stage.name, "prefix_end_index": int(stage.prefix_end_index),
                "stage_episode_count": int(st.stage_episode_count), "recent_success_rate": mean[0], "recent_route_ready_hit_rate": mean[1],
                "recent_orientation_hit_rate": mean[2], "recent_regression_rate": mean[3], "history": history}

    def _destroy(self) -> None:
        self.env.L.kp1_route_curriculum_destroy(self.env._handle, self._st)


class RoutePrefixCurriculumPopulation(TrackerPopulation, RoutePrefixCurriculumDevice):
    """K device trackers, one per replica of a RoutePopulationVecEnv (include/kp1_route.h, kp1_route_curriculum_*_population).  ONE
    ``observe(dones[K N])`` launch per env step: workgroup k scans replica k's envs in env order, advances its clock by N and on promotion moves
    replica k's reset window only.  ``read(k)`` / ``summary(k)`` are RoutePrefixCurriculumDevice's of replica k; ``replica(k)`` is a view
    with read() / summary() for the per-replica lists of a population run.  There is no data-parallel (chunk) form."""

    def attach(self, env: RoutePopulationVecEnv) -> None:
        """_on_training_start of every replica: K trackers next to the population env, every window set to the first prefix"""
        if not isinstance(env, RoutePopulationVecEnv):
            raise TypeError("RoutePrefixCurriculumPopulation tracks the replicas of a RoutePopulationVecEnv")
        env._windows = [self._create(env, env.L.kp1_route_curriculum_create_population)] * env.K

    @property
    def K(self) -> int:
        return self.env.K

    def observe(self, dones: torch.Tensor, steps_per_call: int) -> None:
        """dones: the K N done bytes of one population step; steps_per_call: env steps per replica this call stands for (N)"""
        self._check_done_bytes(dones, dones.numel() == self.env.n_envs)
        native.check(self.env.L.kp1_route_curriculum_observe_population(self.env._handle, self._st, native.ptr(dones), int(steps_per_call),
                                                                        self._stream()))

    def _read_call(self, k: int, out: Any, stream: C.c_void_p) -> int:
        return self.env.L.kp1_route_curriculum_read_replica(self.env._handle, self._st, k, out, stream)

    def _follow(self, st: _CurriculumState, k: int) -> None:
        self.env._windows[k] = (1, int(st.prefix_end_index[st.stage_index]))


RouteCurriculumReplica = TrackerReplica


# --------------------------------------------------------------------------------------------- sequential evaluator
PolicyFn = Callable[[torch.Tensor], torch.Tensor]


def _roll_one(env: RouteVecEnv, policy: PolicyFn, *, initial_q: np.ndarray, goal_index: int, initial_dq: np.ndarray, initial_prev_action: np.ndarray,
              success_dwell_steps: int) -> dict[str, Any]:
    obs = env.reset(options={"route_index": int(goal_index), "start_route_index": 0, "initial_q": initial_q[None], "initial_dq": initial_dq[None],
                             "initial_prev_action": initial_prev_action[None], "evaluator_state": True})
    info = env.info()
    min_pos = float(info["position_error_norm"][0])
    min_ori = float(info["orientation_error_norm"][0])
    min_q = float(np.linalg.norm(env.route_q[min(max(goal_index, 0), env.n_waypoints - 1)] - env.get_state()["q"][0]))
    first_ready_step = None
    max_ready_streak = 0
    steps = 0
    done = 0
    # the episode is a serial dependency chain (one env, the next waypoint starts where this one ends): per step ONE device -> host copy of
    # the eight scalars the bookkeeping needs (f64, exact) instead of one synchronising read per scalar
    keys = ("position_error_norm", "orientation_error_norm", "route_q_error_norm", "route_ready", "route_ready_streak", "action_l2", "executed_delta_q_l2")
    pos = ori = qerr = act = dqn = 0.0
    while not (done & 3):
        action = policy(obs)
        obs, _, d = env.step(action, auto_reset=False)
        info = env.info()
        row = torch.stack([info[k][0].double() for k in keys] + [d[0].double()]).cpu().tolist()
        pos, ori, qerr, ready, streak, act, dqn = row[:7]
        done = int(row[7])
        steps += 1
        min_pos, min_ori, min_q = min(min_pos, pos), min(min_ori, ori), min(min_q, qerr)
        if ready != 0.0 and first_ready_step is None:
            first_ready_step = steps
        max_ready_streak = max(max_ready_streak, int(streak))
    if steps == 0:   # (cannot happen: a fresh episode is never done) keep the row well defined
        pos, ori, qerr = float(info["position_error_norm"][0]), float(info["orientation_error_norm"][0]), float(info["route_q_error_norm"][0])
        act, dqn = float(info["action_l2"][0]), float(info["executed_delta_q_l2"][0])
    st = env.get_state()
    return {
        "route_index": int(goal_index), "success": bool(done & 4), "route_ready_hit": bool(first_ready_step is not None),
        "route_ready_dwell": bool(max_ready_streak >= success_dwell_steps), "first_ready_step": first_ready_step, "max_ready_streak": int(max_ready_streak),
        "steps": int(steps), "final_position_error": float(pos), "final_orientation_error": float(ori), "final_q_error": float(qerr),
        "min_position_error": float(min_pos), "min_orientation_error": float(min_ori), "min_q_error": float(min_q),
        "final_action_magnitude": float(act), "final_dq_norm": float(dqn),
        "final_q": st["q"][0].copy(), "final_dq": st["dq"][0].copy(), "final_prev_action": st["prev_action"][0].copy(),
    }


# first matching rule names why a waypoint failed (eval_route_curriculum.py:113-124): (label, row key, limit); a value above its limit matches
_FAILURE_RULES = (("position", "final_position_error", 0.010), ("orientation", "final_orientation_error", 0.150),
                  ("motion_action", "final_action_magnitude", 1.20), ("motion_action", "final_dq_norm", 0.040), ("q_error", "final_q_error", 0.500))
_ROUTE_CHUNKS = np.array([1, 41, 81, 121, 181, 261, 361, 484])       # chunk c covers route indices [_ROUTE_CHUNKS[c], _ROUTE_CHUNKS[c + 1])
_ROW_MEANS = ("final_position_error", "final_orientation_error", "final_q_error")


def _failure_reason(row: dict[str, Any]) -> str:
    for label, key, limit in _FAILURE_RULES:
        if float(row.get(key, 0.0)) > limit:
            return label
    return "unknown" if row["route_ready_dwell"] else "dwell_or_motion"


def _row_columns(rows: list[dict[str, Any]]) -> dict[str, np.ndarray]:
    """the per-waypoint rows of a sequential evaluation as columns"""
    flags = {k: np.fromiter((bool(r[k]) for r in rows), dtype=bool, count=len(rows)) for k in ("success", "route_ready_hit", "route_ready_dwell")}
    reals = {k: np.fromiter((float(r[k]) for r in rows), dtype=np.float64, count=len(rows)) for k in _ROW_MEANS}
    return {**flags, **reals, "route_index": np.fromiter((int(r["route_index"]) for r in rows), dtype=np.int64, count=len(rows))}


def summarize_rows(rows: list[dict[str, Any]], route_progress_m: np.ndarray) -> dict[str, Any]:
    """route_eval_sequential_summary.json: rates over all targets, the unbroken success prefix from the start and the route length it covers,
    the first failed waypoint and why, mean / max final errors"""
    if not rows:
        return {"target_count": 0}
    col = _row_columns(rows)
    failed = np.flatnonzero(~col["success"])
    prefix = int(failed[0]) if failed.size else len(rows)
    reached = min(prefix, len(route_progress_m) - 1)
    out: dict[str, Any] = {"target_count": len(rows)}
    out.update({name: float(col[key].mean()) for name, key in (("success_rate", "success"), ("route_ready_hit_rate", "route_ready_hit"),
                                                               ("route_ready_dwell_rate", "route_ready_dwell"))})
    out["longest_success_prefix"] = prefix
    out["cumulative_successful_route_distance_m"] = float(route_progress_m[reached] - route_progress_m[0])
    out["first_failure_index"] = int(col["route_index"][failed[0]]) if failed.size else None
    out["first_failure_reason"] = _failure_reason(rows[int(failed[0])]) if failed.size else None
    out.update({f"mean_{k}": float(col[k].mean()) for k in _ROW_MEANS})
    out.update({f"max_{k}": float(col[k].max()) for k in _ROW_MEANS[:2]})
    return out


def chunk_metrics(rows: list[dict[str, Any]]) -> dict[str, Any]:
    """route_chunk_metrics.json: the same rates per fixed stretch of the route (chunks without a target are left out)"""
    if not rows:
        return {}
    col = _row_columns(rows)
    which = np.digitize(col["route_index"], _ROUTE_CHUNKS) - 1
    out: dict[str, Any] = {}
    for c in range(len(_ROUTE_CHUNKS) - 1):
        sel = which == c
        if not sel.any():
            continue
        entry: dict[str, Any] = {"target_count": int(sel.sum()), "success_rate": float(col["success"][sel].mean()),
                                 "route_ready_hit_rate": float(col["route_ready_hit"][sel].mean())}
        entry.update({f"mean_{k}": float(col[k][sel].mean()) for k in _ROW_MEANS})
        out[f"chunk_{c}_{int(_ROUTE_CHUNKS[c])}_{int(_ROUTE_CHUNKS[c + 1]) - 1}"] = entry
    return out


def evaluate_sequential_route(*, policy: PolicyFn | Callable[[RouteVecEnv], PolicyFn], cfg: dict[str, Any], route_q: np.ndarray,
                              artifact_root: str | Path | None = None, end_index: int | None = None, start_index: int = 1, device: int = 0,
                              real: str = "f32", policy_needs_env: bool = False) -> dict[str, Any]:
    """evaluate_sequential_route with the policy passed as a callable obs[1, obs_dim] -> action[1, 7] (checkpoint loading is the
    caller's).  Always the single-waypoint env (``_make_route_env``), whatever ``route.sequence`` says."""
    W = int(route_q.shape[0])
    final_end = min(int(end_index or (W - 1)), W - 1)
    seq_off = {**cfg, "route": {**(cfg.get("route", {}) or {}), "sequence": {**((cfg.get("route", {}) or {}).get("sequence", {}) or {}), "enabled": False}}}
    base = kcfg.to_env_config(cfg)
    env = RouteVecEnv(base, rcfg.route_config_from_dict(seq_off, max_route_index=end_index or (W - 1)), route_q, 1, device=device, seed=0, real=real)
    fn = policy(env) if policy_needs_env else policy
    rows: list[dict[str, Any]] = []
    cq = np.asarray(route_q[max(start_index - 1, 0)], dtype=float).copy()
    cdq = np.zeros_like(cq)
    cpa = np.zeros_like(cq)
    dwell = int(base.c.termination.success_dwell_steps)
    for idx in range(int(start_index), final_end + 1):
        row = _roll_one(env, fn, initial_q=cq, goal_index=idx, initial_dq=cdq, initial_prev_action=cpa, success_dwell_steps=dwell)
        rows.append({k: v for k, v in row.items() if k not in {"final_q", "final_dq", "final_prev_action"}})
        cq, cdq, cpa = row["final_q"], row["final_dq"], row["final_prev_action"]
    progress = env.route_progress_m.copy()
    env.close()
    return sequential_result(rows, progress, start_index=int(start_index), end_index=int(final_end), final_q=cq, artifact_root=artifact_root)


_SEQUENTIAL_EXTRA = ("rows", "chunk_metrics", "final_q")


def sequential_result(rows: list[dict[str, Any]], route_progress_m: np.ndarray, *, start_index: int, end_index: int, final_q,
                      artifact_root: str | Path | None = None) -> dict[str, Any]:
    """what evaluate_sequential_route returns for the per-waypoint ``rows`` of one chain, and its four files under ``artifact_root``
    (summary, chunk metrics, the per-waypoint jsonl and the failure report)"""
    summary = summarize_rows(rows, route_progress_m)
    summary.update({"schema_version": "v5.route_curriculum.sequential_eval.v1", "mode": "sequential_actual_final_q_to_next_dense_q_goal",
                    "start_index": int(start_index), "end_index": int(end_index)})
    if artifact_root is not None:
        root = Path(artifact_root)
        root.mkdir(parents=True, exist_ok=True)
        (root / "route_eval_sequential_summary.json").write_text(json.dumps(summary, indent=2))
        (root / "route_chunk_metrics.json").write_text(json.dumps(chunk_metrics(rows), indent=2))
        with (root / "route_eval_sequential_steps.jsonl").open("w", encoding="utf-8") as fh:
            for row in rows:
                fh.write(json.dumps(row, sort_keys=True) + "\n")
        failure = next((row for row in rows if not row["success"]), None)
        (root / "route_failure_report.json").write_text(json.dumps({"first_failure_index": summary["first_failure_index"],
                                                                    "first_failure_reason": summary["first_failure_reason"], "first_failure": failure}, indent=2))
    return {**summary, "rows": rows, "chunk_metrics": chunk_metrics(rows), "final_q": np.asarray(final_q).tolist()}


# --------------------------------------------------------------------------------------------- chained evaluation of many rows at once
_ALIVE_CHECK_EVERY = 32     # lock steps between two reads of the device's alive counter (the only host synchronisation of the loop)
CHAIN_FORMS = ("launch_sequence", "one_launch_step", "whole_chain")
# what evaluate_sequential_route_batch(form=None) takes where chain_fused_covered says yes (elsewhere the launch sequence, silently).  Chosen
# by measurement (profiles/route_chain_fused.json): both one-launch forms beat the launch sequence's median by more
# than its own spread at K = 1, 8, 16, and one launch per lock step is the faster of the two.  All forms give the same rows, summaries and
# files, bit for bit.
CHAIN_FORM_DEFAULT = "one_launch_step"
CHAIN_FUSED_WIDTHS = (64, 128)
CHAIN_FUSED_MAX_WAYPOINTS = native.header_int("KP1_ROUTE_FUSED_MAX_WAYPOINTS")
CHAIN_RUN_MAX_STEPS = native.ROUTE_CHAIN_RUN_MAX_STEPS


def chain_fused_covered(dtype: Any, hidden: int, obs_dim: int, pitch: int, components_on: bool, n_waypoints: int) -> bool:
    """Whether the chained evaluator's lock step runs as ONE launch (RouteChain.forward_step / RouteChain.run): an fp32 handle, hidden
    64 / 128, the 56-float observation at pitch 56 / 64 or the 80-float one at pitch 80 / 128, reward components off and a route of at
    most CHAIN_FUSED_MAX_WAYPOINTS waypoints.  Plain values only: no handle is touched."""
    if dtype != torch.float32 or int(hidden) not in CHAIN_FUSED_WIDTHS or components_on:
        return False
    if (int(obs_dim), int(pitch)) not in ((56, 56), (56, 64), (80, 80), (80, 128)):
        return False
    return int(n_waypoints) <= CHAIN_FUSED_MAX_WAYPOINTS


def chain_form_selected(form: str | None, covered: bool) -> str:
    """the form evaluate_sequential_route_batch runs: ``None`` takes CHAIN_FORM_DEFAULT and falls back silently to the launch sequence where
    the one-launch kernels do not cover the handles; a form asked for by name and not covered raises"""
    if form is not None and form not in CHAIN_FORMS:
        raise ValueError(f"form must be None or one of {CHAIN_FORMS}, got {form!r}")
    if form is None:
        return CHAIN_FORM_DEFAULT if (covered or CHAIN_FORM_DEFAULT == "launch_sequence") else "launch_sequence"
    if form != "launch_sequence" and not covered:
        raise ValueError(f"form={form!r} needs the one-launch chain kernels: an fp32 route handle, hidden 64 / 128, the 56- or 80-float "
                         "observation at its own or its padded pitch, reward components off and at most "
                         f"{CHAIN_FUSED_MAX_WAYPOINTS} waypoints (form=None falls back to the launch sequence)")
    return form


def chain_lock_steps(needed: int, steps_per_launch: int, bound: int) -> int:
    """lock steps ISSUED by the whole-chain form for a chain whose last row ends at lock step ``needed``: whole spans of ``steps_per_launch``
    until the alive counter reads zero, never past ``bound``"""
    span = max(int(steps_per_launch), 1)
    return min(-(-int(needed) // span) * span, int(bound))


def rows_from_chain_records(records: np.ndarray, route_q: np.ndarray, success_dwell_steps: int) -> list[dict[str, Any]]:
    """the evaluator's per-waypoint rows (_roll_one's keys and order) from one row's chain records (route_env.CHAIN_RECORD).  The device
    keeps the minimum joint error over the episode's steps; the start state's error is formed here from the record's ``start_q`` with
    _roll_one's own 1-D ``np.linalg.norm`` call, so the field is the same double."""
    W = int(route_q.shape[0])
    rows = []
    for rec in records:
        idx = int(rec["route_index"])
        first = int(rec["first_ready_step"])
        start_err = float(np.linalg.norm(route_q[min(max(idx, 0), W - 1)] - rec["start_q"]))
        streak = int(rec["max_ready_streak"])
        rows.append({
            "route_index": idx, "success": bool(rec["success"]), "route_ready_hit": bool(rec["route_ready_hit"]),
            "route_ready_dwell": bool(streak >= success_dwell_steps), "first_ready_step": first if first >= 0 else None, "max_ready_streak": streak,
            "steps": int(rec["steps"]), "final_position_error": float(rec["final_position_error"]),
            "final_orientation_error": float(rec["final_orientation_error"]), "final_q_error": float(rec["final_q_error"]),
            "min_position_error": float(rec["min_position_error"]), "min_orientation_error": float(rec["min_orientation_error"]),
            "min_q_error": min(start_err, float(rec["min_q_error"])), "final_action_magnitude": float(rec["final_action_magnitude"]),
            "final_dq_norm": float(rec["final_dq_norm"])})
    return rows


def check_chain_request(*, replicas: int, n_waypoints: int, start_index, end_indices, rows_per_replica: int) -> tuple[np.ndarray, np.ndarray]:
    """the host-side refusals of evaluate_sequential_route_batch, before any device work; returns (start, end) per row"""
    C_ = int(rows_per_replica)
    if C_ < 1:
        raise ValueError("rows_per_replica must be positive")
    end = np.asarray(end_indices, dtype=np.int64).reshape(-1)
    if end.size != int(replicas) * C_:
        raise ValueError(f"end_indices holds {end.size} chains for a policy handle of {int(replicas)} replicas x {C_} rows per replica "
                         f"(expected {int(replicas) * C_}, replica-major)")
    start = np.broadcast_to(np.asarray(start_index, dtype=np.int64), end.shape)
    if (start < 1).any():
        raise ValueError("start_index must be at least 1 (waypoint 0 is where the route starts)")
    if (end < start).any() or (end >= int(n_waypoints)).any():
        raise ValueError(f"end index out of range: every chain needs start_index <= end_index <= {int(n_waypoints) - 1} (got {end.tolist()})")
    return start.astype(np.int32), end.astype(np.int32)


def evaluate_sequential_route_batch(*, mlp, cfg: dict[str, Any], route_q: np.ndarray, start_index=1, end_indices: Sequence[int],
                                    rows_per_replica: int = 1, device: int | torch.device = 0, artifact_roots: Sequence[str | Path | None] | None = None,
                                    form: str | None = None, steps_per_launch: int = _ALIVE_CHECK_EVERY, **single_only: Any) -> list[dict[str, Any]]:
    """evaluate_sequential_route for K * C chains in lock step: ``mlp`` is a kp1_mlp wrapper (mlp.MlpKernels) of K replicas whose packed
    weights are the policies under test; row r = k C + c runs waypoints ``start_index .. end_indices[r]`` under replica k's policy.  One f32
    route handle of K C envs with ``sequence`` forced off; per lock step one policy forward over all rows and one kp1_route_chain_step, and
    the alive counter is read every _ALIVE_CHECK_EVERY steps.  Returns, per row, what evaluate_sequential_route returns, plus ``final_qs``
    (the final q of every waypoint, for sliced_evaluate) and ``lock_steps``.

    ``form``: "launch_sequence" (the loop above), "one_launch_step" (RouteChain.forward_step: forward, step and hand-over of a lock step in
    one launch) or "whole_chain" (RouteChain.run: ``min(steps_per_launch, remaining bound)`` lock steps per launch, the alive counter read
    after each); ``None`` takes CHAIN_FORM_DEFAULT and falls back silently to the launch sequence where chain_fused_covered says no, a form
    given by name that is not covered raises ValueError.  The three forms give equal rows, summaries and files.  ``lock_steps`` is the count
    of lock steps ISSUED: with ``steps_per_launch`` = 32 (the default) the whole-chain form reports the launch-sequence form's value
    exactly, with a larger span that count rounded up to the span (and never more than the bound)."""
    if single_only:
        raise TypeError(f"evaluate_sequential_route_batch takes packed policy handles and per-row end indices; {sorted(single_only)} belong to "
                        "evaluate_sequential_route (one policy callable, one chain)")
    route_q = np.ascontiguousarray(route_q, dtype=np.float64)
    W = int(route_q.shape[0])
    K, C_ = int(mlp.replicas), int(rows_per_replica)
    start, end = check_chain_request(replicas=K, n_waypoints=W, start_index=start_index, end_indices=end_indices, rows_per_replica=C_)
    R = K * C_
    if artifact_roots is not None and len(artifact_roots) != R:
        raise ValueError(f"{len(artifact_roots)} artifact roots for {R} chains")
    if C_ > int(mlp.max_batch):
        raise ValueError(f"rows_per_replica {C_} exceeds the policy handle's max_batch {int(mlp.max_batch)}")
    seq_off = {**cfg, "route": {**(cfg.get("route", {}) or {}), "sequence": {**((cfg.get("route", {}) or {}).get("sequence", {}) or {}), "enabled": False}}}
    rc = rcfg.route_config_from_dict(seq_off, max_route_index=int(end.max()))
    obs_dim = rcfg.ROUTE_OBS_DIM if rc.include_route_keys else kcfg.OBS_DIM
    if int(mlp.obs_dim) != obs_dim:
        raise ValueError(f"the policy handle reads {int(mlp.obs_dim)}-float observations, the route config produces {obs_dim}")
    # the handle below is fp32 at the policy handle's padded pitch, reward components off: decided before any device work
    form = chain_form_selected(form, chain_fused_covered(torch.float32, int(mlp.hidden), obs_dim, int(mlp.obs_pad), False, W))
    span = int(steps_per_launch)
    if form == "whole_chain" and not 1 <= span <= CHAIN_RUN_MAX_STEPS:
        raise ValueError(f"steps_per_launch must be in [1, {CHAIN_RUN_MAX_STEPS}], got {span}")
    base = kcfg.to_env_config(cfg)
    env = RouteVecEnv(base, rc, route_q, R, device=device, seed=0, real="f32")
    chain = None
    try:
        # every row's two PCG64 streams start as the single evaluator's env does (default_rng(0), env 0); nothing in a chain draws from them
        words = np.repeat(env.rng_state()[:1], R, axis=0)
        env.set_rng_state(words)
        env.base.set_rng_state(np.repeat(env.base.rng_state()[:1], R, axis=0))
        env.use_current_stream()
        pitch = int(mlp.obs_pad)
        env.set_obs_stride(pitch)
        dev = env.device
        obs = torch.zeros((R, pitch), dtype=torch.float32, device=dev)
        act = torch.zeros((R, kcfg.NJ), dtype=torch.float32, device=dev)
        reward = torch.zeros(R, dtype=torch.float32, device=dev)
        done = torch.zeros(R, dtype=torch.uint8, device=dev)
        chain = env.chain(start, end)
        max_steps = max(int(base.c.termination.max_episode_steps), 1)
        bound = int((end - start + 1).max()) * max_steps
        chain.begin(obs)
        steps = 0
        if form == "whole_chain":
            while steps < bound:
                n = min(span, bound - steps)
                chain.run(mlp, obs, reward, done, n)
                steps += n
                if chain.alive() == 0:
                    break
        else:
            while steps < bound:
                if form == "one_launch_step":
                    chain.forward_step(mlp, obs, obs, reward, done)
                else:
                    mlp.forward(obs, clipped=act)
                    chain.step(act, obs, reward, done)
                steps += 1
                if steps % _ALIVE_CHECK_EVERY == 0 and chain.alive() == 0:
                    break
        records = chain.records()
        progress = env.route_progress_m.copy()
    finally:
        if chain is not None:
            chain.close()
        env.close()
    dwell = int(base.c.termination.success_dwell_steps)
    out = []
    for r in range(R):
        rows = rows_from_chain_records(records[r], route_q, dwell)
        if len(rows) != int(end[r]) - int(start[r]) + 1:
            raise native.Kp1Error(f"chain {r} finished {len(rows)} of {int(end[r]) - int(start[r]) + 1} waypoints inside the step bound")
        result = sequential_result(rows, progress, start_index=int(start[r]), end_index=int(end[r]), final_q=records[r][-1]["final_q"],
                                   artifact_root=None if artifact_roots is None else artifact_roots[r])
        result["final_qs"] = [rec["final_q"].tolist() for rec in records[r]]     # per waypoint: what a sliced evaluation reports as final_q
        result["lock_steps"] = steps
        out.append(result)
    return out


def sliced_evaluate(rows: list[dict[str, Any]], final_qs: Sequence[Any], route_progress_m: np.ndarray, *, chain_start: int = 1
                    ) -> Callable[..., dict[str, Any]]:
    """the ``evaluate(artifact_root=, start_index=, end_index=)`` callable of _write_run_artifacts / evaluate_route_gate bound to ONE chain's
    rows: with ``sequence`` off an explicit reset never reads the reset window, so the evaluation to ``end_index`` is the first
    ``end_index - start + 1`` rows of the evaluation to any larger index (tests/test_route_chain_gpu.py proves the prefix property).
    ``final_qs[j]``: the final q of row j."""
    last = len(route_progress_m) - 1

    def evaluate(*, artifact_root: str | Path | None, start_index: int, end_index: int | None) -> dict[str, Any]:
        if int(start_index) != int(chain_start):
            raise ValueError(f"the chain started at waypoint {chain_start}; an evaluation from {start_index} is not a slice of it")
        end_index = min(int(end_index or last), last)     # evaluate_sequential_route's clamp
        count = int(end_index) - int(chain_start) + 1
        if not 1 <= count <= len(rows):
            raise ValueError(f"end_index {end_index} lies outside the chain ({chain_start} .. {chain_start + len(rows) - 1})")
        out = sequential_result(rows[:count], route_progress_m, start_index=int(start_index), end_index=int(end_index), final_q=final_qs[count - 1],
                                artifact_root=artifact_root)
        return {k: v for k, v in out.items() if k not in _SEQUENTIAL_EXTRA}

    return evaluate


# --------------------------------------------------------------------------------------------- sequential gate
def evaluate_route_gate(*, evaluate: Callable[..., dict[str, Any]], artifact_root: str | Path, prefixes: Sequence[int], full_end_index: int | None,
                        min_prefix120_success_rate: float, best_full_longest_prefix: int, full_prefix_tolerance: int, checkpoint: str = "",
                        config: str = "", route_path: str = "") -> dict[str, Any]:
    """Accept or reject a checkpoint from sequential evaluations at several prefixes (eval/eval_route_gate.py:17-99; summary schema
    v5.route_gate.v1).  ``evaluate(artifact_root=, start_index=, end_index=)`` runs one sequential evaluation -- the trainer binds
    evaluate_sequential_route to the policy under test.  A checkpoint passes when it (1) still chains all of prefix 120 at the required
    success rate, (2) gets beyond waypoint 120 on prefix 180, (3) has its first prefix-180 failure after 120, and (4) on the full route
    stays within the tolerance of the best chain length seen so far."""
    root = Path(artifact_root)
    root.mkdir(parents=True, exist_ok=True)
    runs = {f"prefix_{int(p)}": evaluate(artifact_root=root / f"prefix_{int(p)}", start_index=1, end_index=int(p)) for p in prefixes}
    full = None if full_end_index is None else evaluate(artifact_root=root / f"full_{full_end_index}", start_index=1, end_index=int(full_end_index))

    def chain(summary: dict[str, Any] | None) -> int:
        return int(summary.get("longest_success_prefix", 0)) if summary else 0

    at120, at180 = runs.get("prefix_120"), runs.get("prefix_180")
    first_fail_180 = at180.get("first_failure_index") if at180 else 0
    checks = (
        ("prefix120_retention_failed", bool(at120) and chain(at120) >= 120 and float(at120.get("success_rate", 0.0)) >= min_prefix120_success_rate),
        ("prefix180_did_not_expand_beyond_120", bool(at180) and chain(at180) > 120),
        ("prefix180_failed_before_or_at_120", bool(at180) and (first_fail_180 is None or int(first_fail_180) > 120)),
        ("full_route_prefix_regressed_too_much", full is None or chain(full) >= int(best_full_longest_prefix - full_prefix_tolerance)),
    )
    rejected = [reason for reason, ok in checks if not ok]
    summary = {
        "schema_version": "v5.route_gate.v1", "checkpoint": str(checkpoint), "config": str(config), "route_path": str(route_path),
        "accepted": not rejected, "rejection_reasons": rejected,
        "criteria": {"min_prefix120_success_rate": float(min_prefix120_success_rate), "best_full_longest_prefix": int(best_full_longest_prefix),
                     "full_prefix_tolerance": int(full_prefix_tolerance)},
        "prefix_results": runs, "full_result": full,
    }
    (root / "route_gate_summary.json").write_text(json.dumps(summary, indent=2))
    return summary
