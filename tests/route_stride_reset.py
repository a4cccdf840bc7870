"""numpy restatement of the route-stride Approach reset sampler (env.route_reset; the reference's sample_route_approach_reset,
envs/reset_samplers.py:393-423) on a numpy Generator: the CPU yardstick of the lanes the route-stride tests run on ordinary seeds.
tests/golden/route_stride_resets.npz (recorded from the imported reference) pins it bit for bit, test_route_stride_reset_cpu.py.

`settings` is the env.route_reset block of a config (min/max_stride_by_stage, the two noises, reverse_probability); `route_q` the [P, 7]
route; `lower` / `upper` the joint limits; `stage` the env's own, already clamped, stage index."""
from __future__ import annotations

import numpy as np


def sample(rng: np.random.Generator, route_q: np.ndarray, settings: dict, stage: int, lower: np.ndarray, upper: np.ndarray):
    """-> (initial_q, goal_q, start_index, goal_index), draw for draw as the reference"""
    mins, maxs = list(settings.get("min_stride_by_stage", (1,))), list(settings.get("max_stride_by_stage", (1,)))
    s = max(int(stage), 0)
    lo = max(int(mins[min(s, len(mins) - 1)]), 1)
    hi = min(max(int(maxs[min(s, len(maxs) - 1)]), lo), len(route_q) - 1)
    stride = int(rng.integers(lo, hi + 1))                  # a range of one draws nothing
    start = int(rng.integers(0, len(route_q) - stride))
    goal = start + stride
    p = float(settings.get("reverse_probability", 0.0))
    if p > 0.0 and rng.random() < p:
        start, goal = goal, start
    out = []
    for index, key in ((start, "start_q_noise"), (goal, "goal_q_noise")):
        q = np.asarray(route_q[index], dtype=float)
        noise = np.asarray(settings.get(key, [0.0] * 7), dtype=float)
        if np.any(noise > 0.0):
            q = q + rng.uniform(low=-noise, high=noise)
        out.append(np.clip(q, lower, upper))
    return out[0], out[1], start, goal


def draws(n_points: int, settings: dict, stage: int) -> list:
    """the draw sequence of one reset for rng_forcing.classify, up to the start index (the stride is not known before it is drawn, so the
    start-index range is given for a fixed stride only)"""
    mins, maxs = list(settings.get("min_stride_by_stage", (1,))), list(settings.get("max_stride_by_stage", (1,)))
    s = max(int(stage), 0)
    lo = max(int(mins[min(s, len(mins) - 1)]), 1)
    hi = min(max(int(maxs[min(s, len(maxs) - 1)]), lo), n_points - 1)
    seq = [["integers", lo, hi + 1]]
    if lo == hi:
        seq.append(["integers", 0, n_points - lo])
        if float(settings.get("reverse_probability", 0.0)) > 0.0:
            seq.append("double")
    return seq
