"""Done-byte streams and plain restatements for the three curriculum trackers (helper module: no tests in it).

A *stream spec* is a dict of integers (tests/golden/tracker_streams.json stores one per stream next to the reference callbacks' outcomes on
it); ``done_bytes`` / ``flag_planes`` regenerate the stream from the spec, so the fixture holds no stream.  Every draw is a 16-bit value of a
counter hash of (seed, plane, step, env) in 64-bit integer arithmetic: ``_draws`` computes it on uint64 arrays, ``draw_int`` on Python ints,
and the CPU tests compare the two, so the bytes cannot move with the array library.

Spec keys: ``name``, ``tracker`` ("point" / "dock" / "route"), ``seed``, ``T`` steps, ``N`` envs, ``end_q16`` (list, cycled over the steps: an
env ends its episode in step t when its draw is below end_q16[t % len]; 65536 = every env, 0 = none), ``succ`` = {lo, hi, period}: the success
threshold of env i in step t is a triangle wave over the episode position t N + i between lo and hi (all in 1 / 65536), ``flags_q16`` (route:
the thresholds of route_ready, orientation hit and regression) and ``params``, the tracker's settings.

The restatements (PointRule, DockRule, RouteRule) say what PointCurriculumCallback, DockReverseCurriculumCallback and
RoutePrefixCurriculumCallback do with one VecEnv step, in terms of what the device structs expose: stage, stage episode count, the window
oldest first, the clock and the event list.  tests/test_tracker_streams_cpu.py pins them to the reference's outcomes.
"""
from __future__ import annotations

import functools
import json
from collections import deque
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
TERMINATED, TRUNCATED, SUCCESS, INVALID = 1, 2, 4, 8          # include/kp1.h KP1_DONE_*
REC_READY, REC_ORI_HIT, REC_REGRESSION = 16, 32, 64          # include/kp1_route.h KP1_ROUTE_REC_*
FLAG_SET_VALUES = (1, 2, 0x80, 0xFF)                           # what a "set" flag byte holds (0 = clear)
_M = (1 << 64) - 1
_K_SEED, _K_PLANE, _K_STEP, _K_ENV = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0xA0761D6478BD642F, 0xE7037ED1A0B428DB
_MIX1, _MIX2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
# planes of one stream
_P_END, _P_SUCC, _P_KIND, _P_INVALID, _P_IDLE_SUCCESS, _P_FLAG, _P_FLAG_VALUE = 0, 1, 2, 3, 4, 5, 8


# --------------------------------------------------------------------------------------------------------------------- draws
def draw_int(seed: int, plane: int, t: int, i: int) -> int:
    """the 16-bit draw of (seed, plane, step t, env i), on Python integers"""
    z = (seed * _K_SEED + plane * _K_PLANE + t * _K_STEP + i * _K_ENV) & _M
    z = ((z ^ (z >> 30)) * _MIX1) & _M
    z = ((z ^ (z >> 27)) * _MIX2) & _M
    z ^= z >> 31
    z = ((z ^ (z >> 30)) * _MIX1) & _M
    return (z ^ (z >> 29)) >> 48


def _draws(seed: int, plane: int, t: int, n: int) -> np.ndarray:
    """draw_int for envs 0 .. n - 1 at once (uint64 array arithmetic wraps modulo 2^64)"""
    base = np.uint64((seed * _K_SEED + plane * _K_PLANE + t * _K_STEP) & _M)
    z = base + np.arange(n, dtype=np.uint64) * np.uint64(_K_ENV)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_MIX1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(_MIX2)
    z ^= z >> np.uint64(31)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_MIX1)
    return ((z ^ (z >> np.uint64(29))) >> np.uint64(48)).astype(np.int64)


def success_q16(spec: dict, t: int, i):
    """the success threshold of env i (int or int64 array) in step t: a triangle wave over the episode position t N + i"""
    s = spec["succ"]
    period = int(s["period"])
    x = (t * int(spec["N"]) + i) % period
    half = period // 2
    fold = np.minimum(x, period - x) if isinstance(x, np.ndarray) else min(x, period - x)
    return int(s["lo"]) + (int(s["hi"]) - int(s["lo"])) * fold // half


def done_bytes(spec: dict, t: int) -> np.ndarray:
    """uint8[N], the KP1_DONE_* bytes of step t.  An env that ends carries terminated, truncated or both, success by its threshold and the
    invalid bit one time in eight; one that does not end carries success half the time (to be ignored) and the invalid bit as often: every
    value of the low four bits occurs"""
    seed, n = int(spec["seed"]), int(spec["N"])
    ends = spec["end_q16"]
    ended = _draws(seed, _P_END, t, n) < int(ends[t % len(ends)])
    won = _draws(seed, _P_SUCC, t, n) < success_q16(spec, t, np.arange(n, dtype=np.int64))
    kind = _draws(seed, _P_KIND, t, n) % 3 + 1
    invalid = np.where(_draws(seed, _P_INVALID, t, n) < 8192, INVALID, 0)
    idle = np.where(_draws(seed, _P_IDLE_SUCCESS, t, n) < 32768, SUCCESS, 0)
    return (np.where(ended, kind | np.where(won, SUCCESS, 0), idle) | invalid).astype(np.uint8)


def flag_planes(spec: dict, t: int) -> np.ndarray:
    """uint8[3, N]: route_ready, orientation hit, regression of step t, for every env; a set flag holds one of FLAG_SET_VALUES"""
    seed, n = int(spec["seed"]), int(spec["N"])
    values = np.asarray(FLAG_SET_VALUES, dtype=np.int64)
    out = np.zeros((3, n), dtype=np.uint8)
    for q in range(3):
        on = _draws(seed, _P_FLAG + q, t, n) < int(spec["flags_q16"][q])
        out[q] = np.where(on, values[_draws(seed, _P_FLAG_VALUE + q, t, n) % len(values)], 0).astype(np.uint8)
    return out


def record_bytes(done: np.ndarray, flags: np.ndarray) -> np.ndarray:
    """what kp1_route_episode_records writes: the low four done bits | ready << 4 | orientation hit << 5 | regression << 6, flags as != 0"""
    on = (flags != 0).astype(np.uint8)
    return ((done & 0x0F) | (on[0] << 4) | (on[1] << 5) | (on[2] << 6)).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------------- layouts
def rank_blocks(rows: np.ndarray, world: int) -> np.ndarray:
    """[chunk, N] per-step rows of a VecEnv of N = world n_local envs -> the rank-major [world, chunk, n_local] block a data-parallel chunk
    call takes (rank r holds envs r n_local .. (r + 1) n_local - 1)"""
    chunk, n = rows.shape
    assert n % world == 0
    return np.ascontiguousarray(rows.reshape(chunk, world, n // world).transpose(1, 0, 2))


def replica_major(rows: list[np.ndarray]) -> np.ndarray:
    """K per-replica rows [N] -> the [K N] row of a population call (replica k at [k N, (k + 1) N))"""
    assert len({len(r) for r in rows}) == 1
    return np.ascontiguousarray(np.concatenate(rows))


# --------------------------------------------------------------------------------------------------------------------- restatements
class PointRule:
    """One counter, one window of the newest `window` outcomes.  Every finished episode is counted and pushed.  Below the last stage, once the
    stage has seen `min_episodes` episodes and the window is full, a window mean at or above the threshold moves to the next stage: the move
    is logged with the clock, the counter restarts and the window is emptied."""

    def __init__(self, *, threshold: float, window: int, min_episodes: int, max_stage: int, initial_stage: int = 0) -> None:
        self.threshold, self.min_episodes, self.max_stage = float(threshold), max(int(min_episodes), 1), max(int(max_stage), 0)
        self.window = deque(maxlen=max(int(window), 1))
        self.stage = max(min(int(initial_stage), self.max_stage), 0)
        self.count, self.clock = 0, 0
        self.events: list[dict] = []

    def step(self, done: np.ndarray, clock_steps: int, flags: np.ndarray | None = None) -> None:
        self.clock += int(clock_steps)
        for i in np.flatnonzero(done & (TERMINATED | TRUNCATED)):       # envs in index order
            self.count += 1
            self.window.append(1 if done[i] & SUCCESS else 0)
            if self.stage >= self.max_stage or self.count < self.min_episodes or len(self.window) < self.window.maxlen:
                continue
            rate = float(sum(self.window)) / float(len(self.window))
            if rate >= self.threshold:
                self.events.append({"from": self.stage, "to": self.stage + 1, "rate": rate, "total_timesteps": self.clock})
                self.stage += 1
                self.count = 0
                self.window.clear()

    def snapshot(self) -> dict:
        return {"stage": self.stage, "count": self.count, "window": list(self.window), "clock": self.clock, "n_events": len(self.events)}


class DockRule:
    """Stages with their own minimum episode count, threshold and look-back length.  The window keeps the newest `window` outcomes; a stage looks
    at the newest min(its look-back, what the window holds) of them, once the stage has seen its minimum and the window holds
    min(look-back, window) outcomes.  At or above the stage's threshold the next stage starts: logged with the stage's episode count and the
    clock, counter restarted, window emptied.  The last stage only records."""

    def __init__(self, *, stages: list[dict], window: int) -> None:
        self.cap = max(int(window), 1)
        self.stages = [{"min_episodes": max(int(s.get("min_episodes", self.cap)), 1), "threshold": float(s.get("success_rate_threshold", 1.0)),
                        "look_back": max(int(s.get("window_episodes", self.cap)), 1)} for s in stages]
        self.window = deque(maxlen=self.cap)
        self.stage, self.count, self.clock = 0, 0, 0
        self.events: list[dict] = []

    def step(self, done: np.ndarray, clock_steps: int, flags: np.ndarray | None = None) -> None:
        self.clock += int(clock_steps)
        for i in np.flatnonzero(done & (TERMINATED | TRUNCATED)):
            self.count += 1
            self.window.append(1 if done[i] & SUCCESS else 0)
            if self.stage >= len(self.stages) - 1:
                continue
            rule = self.stages[self.stage]
            if self.count < rule["min_episodes"] or len(self.window) < min(rule["look_back"], self.cap):
                continue
            newest = list(self.window)[-min(rule["look_back"], len(self.window)):]
            rate = float(sum(newest)) / float(len(newest))
            if rate >= rule["threshold"]:
                self.events.append({"from": self.stage, "to": self.stage + 1, "rate": rate, "stage_episode_count": self.count,
                                    "total_timesteps": self.clock})
                self.stage += 1
                self.count = 0
                self.window.clear()

    snapshot = PointRule.snapshot


class RouteRule:
    """Four windows side by side (success, ready, orientation hit, regression), one counter.  Once the stage has seen `min_episodes` episodes
    and the windows are full, the three hit rates at or above their thresholds and the regression rate at or below its own ask for the next
    prefix.  On the last stage the request changes nothing: counter and windows carry on.  Otherwise the move is logged with the four rates,
    both prefixes and the clock, the counter restarts and the windows are emptied."""

    def __init__(self, *, prefixes: list[int], success_rate: float, ready_rate: float, orientation_rate: float, max_regression_rate: float,
                 window: int, min_episodes: int) -> None:
        self.prefixes = [int(p) for p in prefixes]
        self.limits = (float(success_rate), float(ready_rate), float(orientation_rate), float(max_regression_rate))
        self.min_episodes = max(int(min_episodes), 1)
        self.windows = [deque(maxlen=max(int(window), 1)) for _ in range(4)]
        self.stage, self.count, self.clock = 0, 0, 0
        self.events: list[dict] = []

    def step(self, done: np.ndarray, clock_steps: int, flags: np.ndarray | None = None) -> None:
        self.clock += int(clock_steps)
        for i in np.flatnonzero(done & (TERMINATED | TRUNCATED)):
            self.count += 1
            outcome = (done[i] & SUCCESS, flags[0][i], flags[1][i], flags[2][i])
            for w, v in zip(self.windows, outcome):
                w.append(1 if v else 0)
            if self.count < self.min_episodes or len(self.windows[0]) < self.windows[0].maxlen:
                continue
            rates = [float(sum(w)) / float(len(w)) for w in self.windows]
            if rates[0] >= self.limits[0] and rates[1] >= self.limits[1] and rates[2] >= self.limits[2] and rates[3] <= self.limits[3] \
                    and self.stage < len(self.prefixes) - 1:
                self.events.append({"from": self.stage, "to": self.stage + 1, "from_prefix": self.prefixes[self.stage],
                                    "to_prefix": self.prefixes[self.stage + 1], "rates": rates, "total_timesteps": self.clock})
                self.stage += 1
                self.count = 0
                for w in self.windows:
                    w.clear()

    def snapshot(self) -> dict:
        return {"stage": self.stage, "count": self.count, "window": [list(w) for w in self.windows], "clock": self.clock, "n_events": len(self.events)}


def make_rule(spec: dict):
    p = spec["params"]
    if spec["tracker"] == "point":
        return PointRule(threshold=p["threshold"], window=p["window"], min_episodes=p["min_episodes"], max_stage=p["max_stage"],
                         initial_stage=p.get("initial_stage", 0))
    if spec["tracker"] == "dock":
        return DockRule(stages=p["stages"], window=p["window"])
    return RouteRule(prefixes=p["prefixes"], success_rate=p["success_rate"], ready_rate=p["ready_rate"], orientation_rate=p["orientation_rate"],
                     max_regression_rate=p["max_regression_rate"], window=p["window"], min_episodes=p["min_episodes"])


def window_len(snapshot: dict) -> int:
    w = snapshot["window"]
    return len(w[0]) if w and isinstance(w[0], list) else len(w)


def replay(spec: dict) -> tuple[list[dict], list[dict]]:
    """the restatement on the whole stream, one VecEnv step at a time (clock += N): (snapshot after every step, events)"""
    rule = make_rule(spec)
    route = spec["tracker"] == "route"
    snaps = []
    for t in range(int(spec["T"])):
        rule.step(done_bytes(spec, t), int(spec["N"]), flag_planes(spec, t) if route else None)
        snaps.append(rule.snapshot())
    return snaps, rule.events


@functools.lru_cache(maxsize=None)
def fixture() -> dict:
    """{stream name: {"spec", "stage", "count", "window_len", "window", "history", "num_timesteps"}}: the reference callbacks' outcomes"""
    raw = json.loads((GOLDEN / "tracker_streams.json").read_text())
    for s in raw["streams"]:
        s["spec"]["params"] = raw["params"][s["spec"]["params"]]              # the file holds each set of settings once
        columns = s["history"]                                                # and the reference's event dicts as columns
        s["history"] = [dict(zip(columns, row)) for row in zip(*columns.values())]
    return {s["spec"]["name"]: s for s in raw["streams"]}


@functools.lru_cache(maxsize=None)
def replay_named(name: str) -> tuple[list[dict], list[dict]]:
    """replay() of a fixture stream, computed once per process; callers leave it unchanged"""
    return replay(fixture()[name]["spec"])
