"""The plain restatements of the three curriculum callbacks (tests/tracker_streams.py) against the reference's own outcomes: on the streams of
tests/golden/tracker_streams.json at every step and in every field, and on the older small traces.  Then the conditions the fixture must
meet for the GPU tests (tests/test_tracker_streams_gpu.py) to reach the kernels' paths, asserted on the reference's outcomes alone.  Every
number compared is an integer or an int / int double: exact equality throughout."""
from __future__ import annotations

import json
import re
from pathlib import Path

import numpy as np
import pytest

import tracker_streams as ts

GOLDEN = ts.GOLDEN
ROOT = Path(__file__).resolve().parent.parent
NAMES = sorted(ts.fixture())
TRACKERS = ("point", "dock", "route")


def _define(header: str, name: str) -> int:
    return int(re.search(rf"#define\s+{name}\s+(\d+)", (ROOT / "include" / header).read_text()).group(1))


POINT_MAX_HISTORY, POINT_MAX_WINDOW = _define("kp1_ppo.h", "KP1_CURRICULUM_MAX_HISTORY"), _define("kp1_ppo.h", "KP1_CURRICULUM_MAX_WINDOW")


def _by_tracker(tracker: str) -> list[dict]:
    return [s for s in ts.fixture().values() if s["spec"]["tracker"] == tracker]


def _promotions_per_step(s: dict) -> dict[int, int]:
    """{step index: promotions in it}: the clock is (t + 1) N after step t"""
    out: dict[int, int] = {}
    for h in s["history"]:
        t = h["total_timesteps"] // s["spec"]["N"] - 1
        out[t] = out.get(t, 0) + 1
    return out


# --------------------------------------------------------------------------------------------------------------------- the generator
def test_array_draws_equal_integer_draws_and_cover_every_byte_value():
    for seed, plane, t, n in ((100, 0, 0, 70), (331, 9, 199, 33), (2 ** 31 - 1, 4, 7, 5)):
        assert ts._draws(seed, plane, t, n).tolist() == [ts.draw_int(seed, plane, t, i) for i in range(n)]
    spec = ts.fixture()["route_obs_4097"]["spec"]
    done, flags = ts.done_bytes(spec, 0), ts.flag_planes(spec, 0)
    assert done.dtype == np.uint8 and flags.dtype == np.uint8 and flags.shape == (3, 4097)
    assert sorted(set(done.tolist())) == list(range(16))                 # success without an end bit and terminated + truncated included
    i = np.arange(4097)
    assert ts.success_q16(spec, 0, i).tolist()[::517] == [ts.success_q16(spec, 0, int(k)) for k in i[::517]]
    for q in range(3):
        assert sorted(set(flags[q].tolist())) == [0] + sorted(ts.FLAG_SET_VALUES)
    rec = ts.record_bytes(done, flags)
    k = int(np.flatnonzero((flags[0] == 0x80) & (flags[1] == 0) & (flags[2] == 0xFF))[0])
    assert rec[k] == (done[k] & 0x0F) | ts.REC_READY | ts.REC_REGRESSION
    quiet = ts.fixture()["point_quiet_4097"]["spec"]
    assert all(not (ts.done_bytes(quiet, t) & 3).any() and (ts.done_bytes(quiet, t) & 4).any() for t in range(quiet["T"]))


def test_layout_helpers():
    rows = np.arange(3 * 12, dtype=np.uint8).reshape(3, 12)                # 3 steps of 12 envs = 4 ranks of 3
    blocks = ts.rank_blocks(rows, 4)
    assert blocks.shape == (4, 3, 3) and blocks.flags["C_CONTIGUOUS"]
    for r in range(4):
        for t in range(3):
            assert blocks[r, t].tolist() == rows[t, 3 * r:3 * r + 3].tolist()
    assert ts.replica_major([rows[0], rows[2]]).tolist() == rows[0].tolist() + rows[2].tolist()


# --------------------------------------------------------------------------------------------------------------------- restatement vs reference
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference_on_every_stream(name):
    want = ts.fixture()[name]
    snaps, events = ts.replay_named(name)
    spec = want["spec"]
    assert [s["stage"] for s in snaps] == want["stage"]
    assert [s["count"] for s in snaps] == want["count"]
    assert [ts.window_len(s) for s in snaps] == want["window_len"]
    assert [s["clock"] for s in snaps] == [(t + 1) * spec["N"] for t in range(spec["T"])]
    assert snaps[-1]["window"] == want["window"] and snaps[-1]["clock"] == want["num_timesteps"]
    assert len(events) == len(want["history"]) == snaps[-1]["n_events"]
    for e, h in zip(events, want["history"]):
        assert e["total_timesteps"] == h["total_timesteps"]
        if spec["tracker"] == "route":
            prefixes = spec["params"]["prefixes"]
            assert (f"prefix_{prefixes[e['from']]}", f"prefix_{prefixes[e['to']]}") == (h["from_stage"], h["to_stage"])
            assert (e["from_prefix"], e["to_prefix"]) == (h["from_prefix_end_index"], h["to_prefix_end_index"])
            assert e["rates"] == [h["recent_success_rate"], h["recent_route_ready_hit_rate"], h["recent_orientation_hit_rate"], h["recent_regression_rate"]]
        else:
            assert (e["from"], e["to"], e["rate"]) == (h["from_stage_index"], h["to_stage_index"], h["trigger_success_rate"])
            if spec["tracker"] == "dock":
                assert e["stage_episode_count"] == h["stage_episode_count"]


def test_restatement_equals_the_small_point_traces():
    """curriculum_tracker.json: one episode per step"""
    for case in json.loads((GOLDEN / "curriculum_tracker.json").read_text())["cases"]:
        rule = ts.PointRule(threshold=case["threshold"], window=case["window"], min_episodes=case["min_episodes"], max_stage=case["n_stages"] - 1)
        stages, promoted_at = [], []
        for i, s in enumerate(case["successes"]):
            before = len(rule.events)
            rule.step(np.array([ts.TRUNCATED | (ts.SUCCESS if s else 0)], dtype=np.uint8), 1)
            stages.append(rule.stage)
            if len(rule.events) > before:
                promoted_at.append(i)
        assert stages == case["stage_after"] and promoted_at == case["promoted_at"]
        assert [e["rate"] for e in rule.events] == case["trigger_rates"]


def test_restatement_equals_the_small_dock_traces():
    g = json.loads((GOLDEN / "dock_reverse_curriculum.json").read_text())
    for trace in g["traces"]:
        rule = ts.DockRule(stages=g["stages"], window=g["window_episodes"])
        for step in trace["steps"]:
            done = np.array([(ts.TRUNCATED if d else 0) | (ts.SUCCESS if s else 0) for d, s in zip(step["dones"], step["success"])], dtype=np.uint8)
            rule.step(done, len(done))
            assert (rule.stage, rule.count) == (step["stage"], step["count"])
        summary = trace["summary"]
        assert [(e["from"], e["to"], e["rate"], e["stage_episode_count"], e["total_timesteps"]) for e in rule.events] == \
               [(h["from_stage_index"], h["to_stage_index"], h["trigger_success_rate"], h["stage_episode_count"], h["total_timesteps"]) for h in summary["history"]]
        assert float(sum(rule.window)) / float(len(rule.window)) == summary["recent_success_rate"]


def test_restatement_equals_the_small_route_traces():
    for trace in json.loads((GOLDEN / "route_eval.json").read_text())["callback"]:
        rule = ts.RouteRule(prefixes=[20, 40, 80], success_rate=0.75, ready_rate=0.75, orientation_rate=0.85, max_regression_rate=0.30, window=16, min_episodes=24)
        for step in trace["steps"]:
            infos = step["infos"]
            done = np.array([(ts.TERMINATED if d else 0) | (ts.SUCCESS if i["success"] else 0) for d, i in zip(step["dones"], infos)], dtype=np.uint8)
            flags = np.array([[int(i[k]) for i in infos] for k in ("route_ready", "route_orientation_hit", "route_regression")], dtype=np.uint8)
            rule.step(done, len(done), flags)
            assert (rule.stage, rule.count) == (step["stage"], step["count"])
        summary = trace["summary"]
        keys = ("recent_success_rate", "recent_route_ready_hit_rate", "recent_orientation_hit_rate", "recent_regression_rate")
        assert [float(sum(w)) / float(len(w)) for w in rule.windows] == [summary[k] for k in keys]
        assert [(e["from_prefix"], e["to_prefix"], e["total_timesteps"], e["rates"]) for e in rule.events] == \
               [(h["from_prefix_end_index"], h["to_prefix_end_index"], h["total_timesteps"], [h[k] for k in keys]) for h in summary["history"]]


# --------------------------------------------------------------------------------------------------------------------- fixture conditions
def test_a_every_stream_promotes_twice_and_the_quiet_streams_never():
    quiet = [n for n in NAMES if "quiet" in n]
    assert {ts.fixture()[n]["spec"]["tracker"] for n in quiet} == set(TRACKERS)
    for name in NAMES:
        s = ts.fixture()[name]
        if name in quiet:
            assert s["history"] == [] and set(s["count"]) == {0} and s["window"] in ([], [[], [], [], []]) and s["num_timesteps"] == s["spec"]["T"] * s["spec"]["N"]
            assert s["spec"]["end_q16"] == [0]
        else:
            assert len(s["history"]) >= 2, name


@pytest.mark.parametrize("tracker", TRACKERS)
def test_b_a_step_with_two_promotions(tracker):
    assert any(max(_promotions_per_step(s).values(), default=0) >= 2 for s in _by_tracker(tracker))


@pytest.mark.parametrize("tracker", TRACKERS)
def test_c_a_promotion_before_the_last_episode_of_its_step(tracker):
    """episodes follow the step's last promotion: the count after the step is their number, and they sit in a window that started empty"""
    hits = 0
    for s in _by_tracker(tracker):
        for t in _promotions_per_step(s):
            if s["count"][t] > 0:
                assert s["window_len"][t] == min(s["count"][t], s["spec"]["params"]["window"])
                hits += 1
    assert hits >= 1


def test_d_a_point_stream_reaches_the_last_stage_and_keeps_recording():
    hits = []
    for s in _by_tracker("point"):
        last = s["spec"]["params"]["max_stage"]
        at_last = [t for t in range(s["spec"]["T"]) if s["stage"][t] == last]
        if len(at_last) >= 2 and s["count"][at_last[-1]] > s["count"][at_last[0]] > 0:
            assert len(s["history"]) == last - s["spec"]["params"]["initial_stage"]
            hits.append(s["spec"]["name"])
    assert hits


def test_e_a_point_stream_outgrows_the_stored_history():
    assert any(len(s["history"]) > POINT_MAX_HISTORY for s in _by_tracker("point"))


def test_f_a_route_stream_satisfies_the_rule_on_the_last_stage():
    """the window at the end passes all four thresholds with the minimum episode count behind it, on the last stage: nothing was cleared"""
    hits = []
    for s in _by_tracker("route"):
        p = s["spec"]["params"]
        if s["stage"][-1] != len(p["prefixes"]) - 1 or s["count"][-1] < p["min_episodes"] or s["window_len"][-1] < p["window"]:
            continue
        rates = [float(sum(w)) / float(len(w)) for w in s["window"]]
        if rates[0] >= p["success_rate"] and rates[1] >= p["ready_rate"] and rates[2] >= p["orientation_rate"] and rates[3] <= p["max_regression_rate"]:
            assert s["count"][-1] > p["window"] and len(s["history"]) == len(p["prefixes"]) - 1
            hits.append(s["spec"]["name"])
    assert hits


def test_g_a_dock_stream_with_look_backs_on_both_sides_of_the_window():
    hits = []
    for s in _by_tracker("dock"):
        p = s["spec"]["params"]
        looks = [st["window_episodes"] for st in p["stages"][:-1] if "window_episodes" in st]
        passed = len(s["history"])                                     # stages 0 .. passed - 1 were judged by their own settings
        judged = p["stages"][:passed]
        if any(st.get("window_episodes", p["window"]) > p["window"] for st in judged) and any(st.get("window_episodes", p["window"]) < p["window"] for st in judged) \
                and any(st.get("min_episodes", 0) > max(looks + [p["window"]]) for st in judged):
            hits.append(s["spec"]["name"])
    assert hits


def test_h_point_blocks_on_both_sides_of_the_whole_wave_threshold():
    many, few = set(), set()
    for s in _by_tracker("point"):
        spec = s["spec"]
        for t in range(spec["T"]):
            ended = (ts.done_bytes(spec, t) & 3) != 0
            for base in range(0, spec["N"], 4096):
                k = int(ended[base:base + 4096].sum())
                (many if k >= 192 else few if k >= 1 else set()).add(spec["name"])
    assert many and few and (many & few)                                # and one stream has both kinds of block


def test_window_sizes_across_the_point_streams():
    sizes = {s["spec"]["params"]["window"] for s in _by_tracker("point")}
    assert {1, 8, POINT_MAX_WINDOW} <= sizes and any(64 % w for w in sizes)
    full = ts.fixture()["point_dense_4096"]["spec"]
    assert full["params"]["window"] == POINT_MAX_WINDOW and full["N"] == 4096 and full["end_q16"][0] == 65536


def test_the_fixture_is_no_larger_than_the_largest_golden_file():
    sizes = {p.name: p.stat().st_size for p in GOLDEN.iterdir() if p.is_file()}
    assert sizes["tracker_streams.json"] <= max(v for k, v in sizes.items() if k != "tracker_streams.json")
