"""The Python half of the three device curriculum trackers without a device: the protocol the families share
(curriculum.DeviceTracker / TrackerPopulation / TrackerReplica) on instances that never ran ``__init__``, every ``_summary_of`` on
hand-filled state mirrors against recorded summaries, and the dock trackers' ``_follow``.

The summaries.  A state mirror is filled from the final state of the plain restatements (tests/tracker_streams.py, pinned to the same
fixtures by tests/test_tracker_streams_cpu.py) after replaying a recorded trace, and ``_summary_of`` must give the trace's recorded
``summary`` (dock: tests/golden/dock_reverse_curriculum.json; route: tests/golden/route_eval.json "callback"; point:
tests/golden/curriculum_tracker.json records none, so the expected dict is built from the restatement's final state).  Every full ring is
filled twice, with ``ring_head`` 0 and with a non-zero head and the contents rotated to match; a ring that is still filling has head 0, as
the device writes it.

Partly filled windows.  Every recorded dock and route trace ENDS on a full window (16 of 16), so the end states alone never reach the
``ring_len < window_episodes`` path.  Each dock and route trace is therefore checked a second time at the last step after which its window
is partly filled (in the promoting traces: just after the last promotion, so with a non-empty history).  No summary is recorded there, so
the expected dict is built as for point: stage, count and window mean from the restatement, and the history rows are the first
``n_events`` rows of the trace's recorded summary.  ``test_fixtures_reach_history_and_partial_windows`` asserts that the cases so formed
hold a non-empty history and a partly filled window for dock and for route."""
from __future__ import annotations

import functools
import json
import types

import numpy as np
import pytest
import torch

import tracker_streams as ts
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import curriculum as cu
from rl_brain_trainer_amd import finisher_tools as ft
from rl_brain_trainer_amd import route_curriculum as rc

GOLDEN = ts.GOLDEN
FAMILIES = ("point", "dock", "route")
K, N = 3, 16


def _bare(cls, **attrs):
    """an instance that never ran __init__ (no device handle behind it)"""
    obj = cls.__new__(cls)
    obj.__dict__.update(attrs)
    return obj


def _population(family: str):
    if family == "point":
        return _bare(cu.PointCurriculumPopulation, K=K)
    if family == "dock":
        return _bare(ft.DockReverseCurriculumPopulation, K=K)
    return _bare(rc.RoutePrefixCurriculumPopulation, env=types.SimpleNamespace(K=K, n_envs=K * N))


# --------------------------------------------------------------------------------------------------------------------- shared protocol
@pytest.mark.parametrize("family", FAMILIES)
def test_replica_is_range_checked(family):
    pop = _population(family)
    for k in (-1, K):
        with pytest.raises(IndexError, match=f"replica {k} of a population of {K}"):
            pop.replica(k)
    view = pop.replica(K - 1)
    assert type(view) is cu.TrackerReplica and view.pop is pop and view.k == K - 1
    assert cu.PointCurriculumReplica is ft.DockReverseCurriculumReplica is rc.RouteCurriculumReplica is cu.TrackerReplica


@pytest.mark.parametrize("family", FAMILIES)
def test_replica_view_is_not_attached_observed_or_closed(family):
    pop = _population(family)
    view = pop.replica(0)
    before = dict(pop.__dict__)
    assert view.attach(None) is None and view.close() is None
    assert pop.__dict__ == before
    with pytest.raises(TypeError, match=f"replica trackers are observed through {type(pop).__name__}.observe"):
        view.observe(torch.zeros(N, dtype=torch.uint8), N)


@pytest.mark.parametrize("family", FAMILIES)
def test_population_has_no_data_parallel_form(family):
    pop = _population(family)
    with pytest.raises(TypeError, match="no data-parallel form"):
        pop.observe_chunk(torch.zeros(2 * 2 * N, dtype=torch.uint8), N, 2, 2)
    if family == "route":
        with pytest.raises(TypeError, match="no data-parallel form"):
            pop.record(torch.zeros(K * N, dtype=torch.uint8), torch.zeros(K * N, dtype=torch.uint8))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("what", ("float32", "non_contiguous", "count"))
def test_population_observe_refuses_before_device_work(family, what):
    """the bare instances have no library, env handle or state behind them: anything past the check would raise AttributeError"""
    pop = _population(family)
    if what == "float32":
        dones = torch.zeros(K * N, dtype=torch.float32)
    elif what == "non_contiguous":
        dones = torch.zeros(2 * K * N, dtype=torch.uint8)[::2]
        assert dones.numel() == K * N and not dones.is_contiguous()
    else:       # not a multiple of K (point, dock); not env.n_envs, though a multiple of K (route)
        dones = torch.zeros(K * N + 1 if family != "route" else K * (N - 1), dtype=torch.uint8)
    with pytest.raises(ValueError, match="contiguous uint8 done bytes"):
        pop.observe(dones, N)


def test_tracker_properties_ppo_reads():
    table = {cu.PointCurriculum: (False, True), cu.PointCurriculumPopulation: (False, True),
             ft.DockReverseCurriculum: (False, False), ft.DockReverseCurriculumPopulation: (False, False),
             rc.RoutePrefixCurriculumDevice: (True, False), rc.RoutePrefixCurriculumPopulation: (False, False)}
    for cls, (records, in_launch) in table.items():
        assert issubclass(cls, cu.DeviceTracker), cls
        assert cls.needs_episode_records is records and cls.runs_in_rollout_launch is in_launch, cls
    assert cu.DeviceTracker.needs_episode_records is False and cu.DeviceTracker.runs_in_rollout_launch is False


# --------------------------------------------------------------------------------------------------------------------- summaries
def _rate(window) -> float:
    return float(sum(window)) / float(len(window)) if len(window) else 0.0


def _snap(rule) -> dict:
    """what a state mirror is filled from: the restatement's state now"""
    windows = [list(w) for w in rule.windows] if hasattr(rule, "windows") else [list(rule.window)]
    return {"stage": rule.stage, "count": rule.count, "clock": rule.clock, "windows": windows, "n_events": len(rule.events)}


def _end_and_last_partial(rule, steps, cap: int) -> list[dict]:
    """replay ``steps`` (an iterable of rule.step argument tuples): the end state, and the state after the last step that left the window
    partly filled (None: no such step)"""
    partial = None
    for args in steps:
        rule.step(*args)
        if 0 < len(_snap(rule)["windows"][0]) < cap:
            partial = _snap(rule)
    return [_snap(rule)] + ([partial] if partial is not None else [])


def _heads(snap: dict, cap: int) -> tuple[int, ...]:
    """the ring heads a state is filled with: 0, and for a full ring two non-zero ones as well"""
    return (0, 1, cap - 1) if len(snap["windows"][0]) == cap and cap > 1 else (0,)


def _fill_common(st, snap: dict, cap: int, head: int, rings) -> None:
    st.stage_index, st.stage_episode_count, st.n_events, st.num_timesteps = snap["stage"], snap["count"], snap["n_events"], snap["clock"]
    st.window_episodes, st.ring_len, st.ring_head = cap, len(snap["windows"][0]), head
    for ring, window in zip(rings, snap["windows"]):
        for slot in range(len(ring)):
            ring[slot] = 1          # dead slots hold stale outcomes on the device too: a mean that reads them shows
        for j, v in enumerate(window):
            ring[(head + j) % cap] = v


@functools.lru_cache(maxsize=None)
def _dock_cases() -> tuple:
    g = json.loads((GOLDEN / "dock_reverse_curriculum.json").read_text())
    names = [s.get("name", f"stage_{i}") for i, s in enumerate(g["stages"])]
    cases = []
    for trace in g["traces"]:
        rule = ts.DockRule(stages=g["stages"], window=g["window_episodes"])
        steps = [(np.array([(ts.TRUNCATED if d else 0) | (ts.SUCCESS if s else 0) for d, s in zip(step["dones"], step["success"])], dtype=np.uint8),
                  len(step["dones"])) for step in trace["steps"]]
        end, *partial = _end_and_last_partial(rule, steps, rule.cap)
        cases.append((end, rule.events, trace["summary"]))
        for snap in partial:
            cases.append((snap, rule.events, {"stage_index": snap["stage"], "stage_name": names[snap["stage"]], "stage_episode_count": snap["count"],
                                              "recent_success_rate": _rate(snap["windows"][0]), "history": trace["summary"]["history"][:snap["n_events"]]}))
    return g, tuple(cases)


ROUTE_PREFIXES, ROUTE_WINDOW = [20, 40, 80], 16
ROUTE_RATES = ("recent_success_rate", "recent_route_ready_hit_rate", "recent_orientation_hit_rate", "recent_regression_rate")


@functools.lru_cache(maxsize=None)
def _route_cases() -> tuple:
    cases = []
    for trace in json.loads((GOLDEN / "route_eval.json").read_text())["callback"]:
        rule = ts.RouteRule(prefixes=ROUTE_PREFIXES, success_rate=0.75, ready_rate=0.75, orientation_rate=0.85, max_regression_rate=0.30,
                            window=ROUTE_WINDOW, min_episodes=24)         # the settings test_restatement_equals_the_small_route_traces replays with
        steps = []
        for step in trace["steps"]:
            infos = step["infos"]
            done = np.array([(ts.TERMINATED if d else 0) | (ts.SUCCESS if i["success"] else 0) for d, i in zip(step["dones"], infos)], dtype=np.uint8)
            flags = np.array([[int(i[k]) for i in infos] for k in ("route_ready", "route_orientation_hit", "route_regression")], dtype=np.uint8)
            steps.append((done, len(done), flags))
        end, *partial = _end_and_last_partial(rule, steps, ROUTE_WINDOW)
        cases.append((end, rule.events, trace["summary"]))
        for snap in partial:
            expected = {"stage_index": snap["stage"], "stage_name": f"prefix_{ROUTE_PREFIXES[snap['stage']]}", "prefix_end_index": ROUTE_PREFIXES[snap["stage"]],
                        "stage_episode_count": snap["count"], **{key: _rate(w) for key, w in zip(ROUTE_RATES, snap["windows"])},
                        "history": trace["summary"]["history"][:snap["n_events"]]}
            cases.append((snap, rule.events, expected))
    return tuple(cases)


def test_fixtures_reach_history_and_partial_windows():
    """the summary tests below cannot pass on empty cases: dock and route each have a case with a non-empty history, one with a partly
    filled window and one with a full one (which is filled at three ring heads)"""
    for cases, cap in ((_dock_cases()[1], _dock_cases()[0]["window_episodes"]), (_route_cases(), ROUTE_WINDOW)):
        assert any(expected["history"] for _, _, expected in cases)
        assert any(0 < len(snap["windows"][0]) < cap for snap, _, _ in cases)
        assert any(0 < len(snap["windows"][0]) < cap and snap["n_events"] for snap, _, _ in cases)
        assert any(len(_heads(snap, cap)) == 3 for snap, _, _ in cases)
        assert any(0 < sum(w) < len(w) for snap, _, _ in cases for w in snap["windows"])       # a mean that is neither 0 nor 1


def test_dock_summary_of_hand_filled_states():
    g, cases = _dock_cases()
    cur = _bare(ft.DockReverseCurriculum, stages=[dict(s) for s in g["stages"]])
    cap = int(g["window_episodes"])
    for snap, events, expected in cases:
        summaries = []
        for head in _heads(snap, cap):
            st = ft._State()
            _fill_common(st, snap, cap, head, [st.ring])
            for e, ev in zip(st.events, events[:snap["n_events"]]):
                e.from_stage, e.to_stage, e.stage_episode_count = ev["from"], ev["to"], ev["stage_episode_count"]
                e.trigger_success_rate, e.total_timesteps = ev["rate"], ev["total_timesteps"]
            summaries.append(json.loads(json.dumps(cur._summary_of(st))))
        assert all(s == expected for s in summaries), (snap, summaries)


def test_route_summary_of_hand_filled_states():
    cur = _bare(rc.RoutePrefixCurriculumDevice, stages=rc.build_prefix_stages(ROUTE_PREFIXES))
    for snap, events, expected in _route_cases():
        summaries = []
        for head in _heads(snap, ROUTE_WINDOW):
            st = rc._CurriculumState()
            _fill_common(st, snap, ROUTE_WINDOW, head, list(st.ring))
            for e, ev in zip(st.events, events[:snap["n_events"]]):
                e.from_stage, e.to_stage, e.from_prefix_end_index, e.to_prefix_end_index = ev["from"], ev["to"], ev["from_prefix"], ev["to_prefix"]
                e.total_timesteps = ev["total_timesteps"]
                e.recent_success_rate, e.recent_route_ready_hit_rate, e.recent_orientation_hit_rate, e.recent_regression_rate = ev["rates"]
            summaries.append(json.loads(json.dumps(cur._summary_of(st))))
        assert all(s == expected for s in summaries), (snap, summaries)


def test_point_summary_of_hand_filled_states():
    reached_full = reached_history = False
    for case in json.loads((GOLDEN / "curriculum_tracker.json").read_text())["cases"]:
        rule = ts.PointRule(threshold=case["threshold"], window=case["window"], min_episodes=case["min_episodes"], max_stage=case["n_stages"] - 1)
        steps = [(np.array([ts.TRUNCATED | (ts.SUCCESS if s else 0)], dtype=np.uint8), 1) for s in case["successes"]]
        cap = int(case["window"])
        for snap in _end_and_last_partial(rule, steps, cap):
            expected = {"stage_index": snap["stage"], "stage_episode_count": snap["count"], "recent_success_rate": _rate(snap["windows"][0]),
                        "history": [{"from_stage_index": ev["from"], "to_stage_index": ev["to"], "trigger_success_rate": ev["rate"],
                                     "total_timesteps": ev["total_timesteps"]} for ev in rule.events[:snap["n_events"]]]}
            for head in _heads(snap, cap):
                st = cu.CurriculumState()
                _fill_common(st, snap, cap, head, [st.ring])
                for e, ev in zip(st.events, rule.events[:snap["n_events"]]):
                    e.from_stage, e.to_stage, e.trigger_success_rate, e.total_timesteps = ev["from"], ev["to"], ev["rate"], ev["total_timesteps"]
                assert cu.PointCurriculum._summary_of(st) == expected, (snap, head)
            reached_full |= len(_heads(snap, cap)) == 3
            reached_history |= bool(expected["history"])
    assert reached_full and reached_history


def test_window_mean_of_an_empty_window_is_zero():
    st = cu.CurriculumState()
    st.window_episodes = 4
    assert cu.window_mean(st, st.ring) == 0.0


# --------------------------------------------------------------------------------------------------------------------- dock _follow
def _dock_config() -> kcfg.EnvConfig:
    return kcfg.to_env_config(kcfg.load_yaml_file(kcfg.builtin_config_dir() / "dock_workspace_handoff_noop_ft_12env.yaml"))


def _live_state(stage_index: int) -> ft._State:
    """a state on ``stage_index`` whose stage records all differ, field by field, from each other and from any config"""
    st = ft._State()
    st.stage_index = stage_index
    for s in range(3):
        for j, key in enumerate(ft._STAGE_ENV_KEYS + ft._STAGE_RESET_SCALARS):
            setattr(st.stages[s], key, 1000.0 * (s + 1) + j + 0.25)
        for j, key in enumerate(ft._STAGE_RESET_VECTORS):
            getattr(st.stages[s], key)[:] = [2000.0 * (s + 1) + 10 * j + i + 0.5 for i in range(kcfg.NJ)]
    return st


def _assert_followed(c, before, live) -> None:
    """``c`` holds the live record's value in every overridable field and ``before``'s bytes everywhere else"""
    for key in ft._STAGE_ENV_KEYS:
        assert getattr(c.env, key) == getattr(live, key), key
        setattr(c.env, key, getattr(before.env, key))
    for key in ft._STAGE_RESET_SCALARS:
        assert getattr(c.dock_reset, key) == getattr(live, key), key
        setattr(c.dock_reset, key, getattr(before.dock_reset, key))
    for key in ft._STAGE_RESET_VECTORS:
        assert list(getattr(c.dock_reset, key)) == list(getattr(live, key)), key
        getattr(c.dock_reset, key)[:] = getattr(before.dock_reset, key)[:]
    assert bytes(c) == bytes(before)


def test_dock_follow_copies_the_live_stage_into_the_env_config():
    cfg = _dock_config()
    before = cfg.clone().c
    cur = _bare(ft.DockReverseCurriculum, env=types.SimpleNamespace(config=cfg))
    st = _live_state(1)
    assert cur._follow(st, 0) is None
    assert bytes(cfg.c) != bytes(before)
    _assert_followed(cfg.c, before, st.stages[1])


def test_dock_population_follow_copies_into_that_replica_s_config_only():
    cfg = _dock_config()
    before = bytes(cfg.c)
    configs = [cfg.clone(), cfg.clone()]
    pop = _bare(ft.DockReverseCurriculumPopulation, K=2, configs=configs, env=types.SimpleNamespace(config=cfg))
    st = _live_state(2)
    pop._follow(st, 1)
    assert bytes(configs[0].c) == before and bytes(cfg.c) == before
    _assert_followed(configs[1].c, cfg.clone().c, st.stages[2])
    assert pop.replica(1).config is configs[1] and pop.replica(0).config is configs[0]
