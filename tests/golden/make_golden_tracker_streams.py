#!/usr/bin/env python3
"""Outcomes of the reference's three curriculum callbacks (training/callbacks.py PointCurriculumCallback and DockReverseCurriculumCallback,
route/route_curriculum.py RoutePrefixCurriculumCallback) on the streams of tests/tracker_streams.py, driven without SB3 (the base class
degrades to ``object``; instances are built without __init__ and given a fake training_env).  Runs ONLY in the build container.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_tracker_streams.py

Writes tracker_streams.json: per stream the spec and the OUTCOMES only (stage, stage episode count and window length after every step, the
final window contents, the full history with its dicts laid out as columns, the final num_timesteps), one stream per line, and every distinct
set of tracker settings once under "params".  The streams themselves are regenerated from the specs.
"""
from __future__ import annotations

import json
import sys
from collections import deque
from pathlib import Path

REF = Path("/root/reference/hrl_ws/src/hrl_trainer")
OUT = Path(__file__).resolve().parent
sys.dont_write_bytecode = True
sys.path.insert(0, str(REF))
sys.path.insert(0, str(OUT.parent))

import tracker_streams as ts  # noqa: E402
from hrl_trainer.kinematic_phase1.route.route_curriculum import RoutePrefixCurriculumCallback, build_prefix_stages  # noqa: E402
from hrl_trainer.kinematic_phase1.training.callbacks import DockReverseCurriculumCallback, PointCurriculumCallback  # noqa: E402


def q16(p: float) -> int:
    return int(round(p * 65536))


ALL, NONE, SPARSE = 65536, 0, q16(0.02)
DRIFT = {"lo": q16(0.55), "hi": q16(0.97), "period": 3000}           # success probability around the 0.75 thresholds
DRIFT_SHORT = {"lo": q16(0.45), "hi": q16(0.99), "period": 90}       # the same for streams of a few hundred episodes


def point(window, min_episodes, max_stage=1000, threshold=0.75, initial_stage=0):
    return {"threshold": threshold, "window": window, "min_episodes": min_episodes, "max_stage": max_stage, "initial_stage": initial_stage}


# stage look-backs on both sides of the tracker window, and a minimum episode count above both (stage 2)
DOCK_A = {"window": 16, "stages": [
    {"name": "close", "dock_residual_action_limit": 0.20, "close_bucket_probability": 1.0, "close_bucket_max_pos_error_m": 0.004,
     "init_q_noise": [0.001] * 7, "min_episodes": 12, "success_rate_threshold": 0.7, "window_episodes": 10},
    {"name": "mid", "action_delta_scale": 0.012, "dock_residual_action_limit": 0.25, "close_bucket_probability": 0.7,
     "handoff_state_probability": 0.5, "min_episodes": 20, "success_rate_threshold": 0.6, "window_episodes": 24},
    {"name": "far", "dock_residual_action_limit": 0.30, "close_bucket_probability": 0.4, "min_episodes": 30, "success_rate_threshold": 0.65},
    {"name": "wide", "dock_delta_q_change_limit_scale": 0.5, "dock_residual_action_limit": 0.35, "close_bucket_probability": 0.1},
]}
DOCK_B = {"window": 48, "stages": [
    {"name": "s0", "dock_residual_action_limit": 0.21, "close_bucket_probability": 0.9, "min_episodes": 50, "success_rate_threshold": 0.7, "window_episodes": 20},
    {"name": "s1", "dock_residual_action_limit": 0.22, "close_bucket_probability": 0.8, "min_episodes": 48, "success_rate_threshold": 0.7, "window_episodes": 100},
    {"name": "s2", "dock_residual_action_limit": 0.23, "close_bucket_probability": 0.7, "min_episodes": 120, "success_rate_threshold": 0.72},
    {"name": "s3", "dock_residual_action_limit": 0.24, "close_bucket_probability": 0.6, "min_episodes": 1, "success_rate_threshold": 0.75, "window_episodes": 1},
    {"name": "s4", "dock_residual_action_limit": 0.26, "close_bucket_probability": 0.5, "success_rate_threshold": 0.8},
    {"name": "s5", "dock_residual_action_limit": 0.27, "close_bucket_probability": 0.3},
]}


def route(window, min_episodes, prefixes=(5, 10, 20, 40), rates=(0.75, 0.75, 0.85, 0.30)):
    return {"prefixes": list(prefixes), "success_rate": rates[0], "ready_rate": rates[1], "orientation_rate": rates[2],
            "max_regression_rate": rates[3], "window": window, "min_episodes": min_episodes}


ROUTE_FLAGS = [q16(0.9), q16(0.95), q16(0.1)]
ROUTE_OPEN = (0.5, 0.5, 0.5, 0.5)       # passes almost always: the stream reaches the last stage and satisfies the rule there


def spec(name, tracker, seed, T, N, end, params, succ=DRIFT, chunk=None):
    s = {"name": name, "tracker": tracker, "seed": seed, "T": T, "N": N, "end_q16": list(end), "succ": dict(succ), "params": params}
    if tracker == "route":
        s["flags_q16"] = list(ROUTE_FLAGS)
    if chunk is not None:
        s["chunk"] = list(chunk)           # (n_local, chunk_steps, world): N = n_local world, T a multiple of chunk_steps
    return s


def specs() -> list[dict]:
    out = []
    # ---- point tracker, observe: at each N every env ends ("dense") and p_end ~ 0.02 ("sparse"), both with steps in which nothing ends
    # (min_episodes keeps the histories short; 4097 is the stream that outgrows the stored history and then sits on the last stage)
    dense_params = {1: point(8, 8), 63: point(20, 80), 64: point(8, 100), 65: point(48, 64), 4095: point(20, 48, max_stage=5), 4096: point(1024, 1100),
                    4097: point(8, 8, max_stage=90), 8200: point(48, 2000)}
    for k, (n, p) in enumerate(dense_params.items()):
        T = 200 if n == 1 else 40 if n < 100 else 8
        out.append(spec(f"point_dense_{n}", "point", 100 + k, T, n, [ALL, ALL, NONE, ALL], p, succ=DRIFT if n > 100 else DRIFT_SHORT))
    for k, n in enumerate(dense_params):
        small = n < 100
        T = 200 if n == 1 else 100 if small else 10
        end = [q16(0.06) if n == 1 else SPARSE, SPARSE, NONE, SPARSE] if n < 100 else [SPARSE, NONE, SPARSE]
        out.append(spec(f"point_sparse_{n}", "point", 120 + k, T, n, end, point(1, 1 if n == 1 else 10, threshold=0.5) if small else point(20 if n != 4096 else 8, 30),
                        succ=DRIFT_SHORT if small else {"lo": q16(0.55), "hi": q16(0.97), "period": 400}))
    out.append(spec("point_mid_8200", "point", 140, 8, 8200, [q16(0.1), q16(0.3), NONE, q16(0.06)], point(20, 20, max_stage=12)))
    out.append(spec("point_quiet_4097", "point", 141, 6, 4097, [NONE], point(8, 8)))
    # ---- point tracker, observe_chunk
    for k, (nl, ch, w, p, end) in enumerate([(64, 4, 2, point(8, 60), [ALL, q16(0.3), NONE]), (100, 3, 3, point(20, 100), [q16(0.5), NONE, ALL, q16(0.1)]),
                                              (4097, 2, 2, point(48, 48, max_stage=15), [q16(0.5), SPARSE, ALL]), (40, 16, 1, point(20, 24), [ALL, NONE, q16(0.2)])]):
        T = {4: 12, 3: 12, 2: 8, 16: 48}[ch]
        out.append(spec(f"point_chunk_{nl}_{ch}_{w}", "point", 150 + k, T, nl * w, end, p, succ=DRIFT if nl > 1000 else DRIFT_SHORT, chunk=(nl, ch, w)))
    # ---- point tracker, population: three streams per N, one of them without any episode
    for n, p, T in ((65, (8, 80), 24), (4096, (20, 1500), 8)):
        out.append(spec(f"point_pop_{n}_a", "point", 160 + n % 7, T, n, [ALL, ALL, NONE, q16(0.5)], point(*p, initial_stage=0), succ=DRIFT if n > 100 else DRIFT_SHORT))
        out.append(spec(f"point_pop_{n}_b", "point", 170 + n % 7, T, n, [NONE, q16(0.4), ALL, q16(0.1)], point(*p, initial_stage=2), succ=DRIFT if n > 100 else DRIFT_SHORT))
        out.append(spec(f"point_quiet_{n}", "point", 180 + n % 7, T, n, [NONE], point(*p, initial_stage=1)))
    # ---- dock reverse tracker
    for k, n in enumerate((5, 8, 12, 65, 4097)):
        big = n > 1000
        out.append(spec(f"dock_obs_{n}", "dock", 200 + k, 8 if big else 40 if n == 65 else 200 if n == 5 else 100, n, [q16(0.3), q16(0.2), NONE], DOCK_B if big else DOCK_A,
                        succ={"lo": q16(0.5), "hi": q16(0.99), "period": 600} if big else DRIFT_SHORT))
    out.append(spec("dock_quiet_12", "dock", 210, 6, 12, [NONE], DOCK_A))
    for k, (nl, ch, w) in enumerate([(12, 4, 2), (65, 3, 3), (4097, 2, 2)]):
        big = nl > 1000
        out.append(spec(f"dock_chunk_{nl}_{ch}_{w}", "dock", 220 + k, 8 if big else 48, nl * w, [q16(0.3), NONE, q16(0.15)], DOCK_B if big else DOCK_A,
                        succ={"lo": q16(0.5), "hi": q16(0.99), "period": 600} if big else DRIFT_SHORT, chunk=(nl, ch, w)))
    for n, T in ((12, 100), (65, 40)):
        for k, end in enumerate(([q16(0.3), q16(0.2), NONE], [NONE, q16(0.4), q16(0.1)], [q16(0.15)])):
            if n == 12 and k == 2:
                continue                   # replica 2 of the 12-env population is dock_quiet_12's twin below
            out.append(spec(f"dock_pop_{n}_{'abc'[k]}", "dock", 230 + 10 * k + n % 7, T, n, end, DOCK_A, succ=DRIFT_SHORT))
    out.append(spec("dock_quiet_12_long", "dock", 250, 100, 12, [NONE], DOCK_A))
    # ---- route prefix tracker
    for k, n in enumerate((3, 4, 5, 67, 4097, 68, 4100)):      # 4-byte words need N % 4 == 0: 68 reaches a second lane, 4100 a second block
        big = n > 1000
        p = route(100, 128, prefixes=(5, 10, 20, 40, 80, 120)) if big else route(16, 24, rates=ROUTE_OPEN, prefixes=(5, 10, 20)) if n == 5 else route(16, 24)
        out.append(spec(f"route_obs_{n}", "route", 300 + k, 6 if big else 40 if n > 60 else 200, n, [q16(0.3), q16(0.2), NONE], p,
                        succ={"lo": q16(0.6), "hi": q16(0.99), "period": 700} if big else {"lo": q16(0.6), "hi": q16(0.99), "period": 90}))
    out.append(spec("route_quiet_5", "route", 310, 6, 5, [NONE], route(16, 24)))
    for k, (nl, ch, w) in enumerate([(64, 4, 2), (100, 3, 3), (4097, 2, 2)]):
        big = nl > 1000
        out.append(spec(f"route_chunk_{nl}_{ch}_{w}", "route", 320 + k, 8 if big else 24, nl * w, [q16(0.3), NONE, q16(0.6)],
                        route(100, 128, prefixes=(5, 10, 20, 40, 80, 120)) if big else route(16, 24),
                        succ={"lo": q16(0.6), "hi": q16(0.99), "period": 700} if big else {"lo": q16(0.6), "hi": q16(0.99), "period": 90}, chunk=(nl, ch, w)))
    for k, end in enumerate(([q16(0.3), q16(0.2), NONE], [NONE, q16(0.5), q16(0.1)], [q16(0.15)])):
        out.append(spec(f"route_pop_67_{'abc'[k]}", "route", 330 + k, 40, 67, end, route(16, 24), succ={"lo": q16(0.6), "hi": q16(0.99), "period": 90}))
    return out


class FakeVecEnv:
    def env_method(self, *a, **kw):
        pass


def reference(s: dict):
    p = s["params"]
    if s["tracker"] == "point":
        cb = object.__new__(PointCurriculumCallback)
        cb.success_rate_threshold, cb.window_episodes, cb.min_episodes_per_stage = float(p["threshold"]), int(p["window"]), int(p["min_episodes"])
        cb.max_stage_index, cb.current_stage_index = int(p["max_stage"]), int(p["initial_stage"])
        cb.recent_successes = deque(maxlen=cb.window_episodes)
        windows = lambda: [cb.recent_successes]  # noqa: E731
    elif s["tracker"] == "dock":
        cb = object.__new__(DockReverseCurriculumCallback)
        cb.stages, cb.window_episodes, cb.current_stage_index = list(p["stages"]), int(p["window"]), 0
        cb.recent_successes = deque(maxlen=cb.window_episodes)
        windows = lambda: [cb.recent_successes]  # noqa: E731
    else:
        cb = object.__new__(RoutePrefixCurriculumCallback)
        cb.stages = build_prefix_stages(p["prefixes"])
        cb.promotion_success_rate, cb.promotion_route_ready_hit_rate = float(p["success_rate"]), float(p["ready_rate"])
        cb.promotion_orientation_hit_rate, cb.promotion_max_regression_rate = float(p["orientation_rate"]), float(p["max_regression_rate"])
        cb.window_episodes, cb.min_episodes_per_stage, cb.current_stage_index = int(p["window"]), int(p["min_episodes"]), 0
        cb.successes, cb.ready_hits = deque(maxlen=cb.window_episodes), deque(maxlen=cb.window_episodes)
        cb.orientation_hits, cb.regressions = deque(maxlen=cb.window_episodes), deque(maxlen=cb.window_episodes)
        windows = lambda: [cb.successes, cb.ready_hits, cb.orientation_hits, cb.regressions]  # noqa: E731
    cb.stage_episode_count, cb.history, cb.training_env, cb.num_timesteps = 0, [], FakeVecEnv(), 0
    cb._on_training_start()
    return cb, windows


def outcomes(s: dict) -> dict:
    cb, windows = reference(s)
    n = int(s["N"])
    stage, count, wlen = [], [], []
    for t in range(int(s["T"])):
        done = ts.done_bytes(s, t)
        flags = ts.flag_planes(s, t) if s["tracker"] == "route" else None
        infos = []
        for i in range(n):
            info = {"success": bool(done[i] & ts.SUCCESS)}
            if flags is not None:
                info.update(route_ready=bool(flags[0][i]), route_orientation_hit=bool(flags[1][i]), route_regression=bool(flags[2][i]))
            infos.append(info)
        cb.num_timesteps += n
        cb.locals = {"infos": infos, "dones": [bool(d & (ts.TERMINATED | ts.TRUNCATED)) for d in done]}
        cb._on_step()
        stage.append(int(cb.current_stage_index))
        count.append(int(cb.stage_episode_count))
        wlen.append(len(windows()[0]))
    w = [list(map(int, x)) for x in windows()]
    history = {key: [h[key] for h in cb.history] for key in (cb.history[0] if cb.history else {})}        # the reference's dicts, as columns
    return {"spec": s, "stage": stage, "count": count, "window_len": wlen, "window": w if s["tracker"] == "route" else w[0],
            "history": history, "num_timesteps": int(cb.num_timesteps)}


def main() -> None:
    streams = [outcomes(s) for s in specs()]
    tables: dict[str, dict] = {}                       # every distinct set of tracker settings once; a spec names its set
    for o in streams:
        text = json.dumps(o["spec"]["params"], sort_keys=True)
        key = next((k for k, v in tables.items() if json.dumps(v, sort_keys=True) == text), f"{o['spec']['tracker']}_{len(tables)}")
        tables[key] = o["spec"]["params"]
        o["spec"] = {**o["spec"], "params": key}
    dump = lambda x: json.dumps(x, separators=(",", ":"))  # noqa: E731
    lines = ['{"params":{'] + [f"{dump(k)}:{dump(v)}" + ("," if i + 1 < len(tables) else "") for i, (k, v) in enumerate(tables.items())] + ['},"streams":[']
    lines += [dump(o) + ("," if i + 1 < len(streams) else "") for i, o in enumerate(streams)] + ["]}"]
    (OUT / "tracker_streams.json").write_text("\n".join(lines) + "\n")
    for o in streams:
        per_step: dict[int, int] = {}
        for clock in o["history"].get("total_timesteps", []):
            per_step[clock] = per_step.get(clock, 0) + 1
        print(f"{o['spec']['name']:24s} promotions {sum(per_step.values()):4d}  most in a step {max(per_step.values(), default=0):3d}  final stage {o['stage'][-1]:4d}"
              f"  count {o['count'][-1]:6d}  window {o['window_len'][-1]}")
    print("bytes", (OUT / "tracker_streams.json").stat().st_size)


if __name__ == "__main__":
    main()
