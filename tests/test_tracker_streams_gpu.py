"""The three device curriculum trackers against the reference callbacks at the shapes where their load paths change.

Every case feeds a stream of tests/tracker_streams.py to one device form through its Python handle and compares ``read()`` after EVERY call
with the plain restatement of the reference callback (stage, stage episode count, window length and live entries oldest first, event count,
clock), and the event history at the end, field by field.  The restatement is pinned to the reference's own outcomes on the same streams by
tests/test_tracker_streams_cpu.py.  Everything compared is an integer or an int / int double: exact equality, no tolerances.

Shapes: the point tracker's 16-byte path needs an aligned run of 64 envs (N = 1, 63: bytewise only; 64, 65: one wave lane + tail; 4095 .. 4097:
a full 4096-env block, a ragged last lane, a second block of one env; 8200: three blocks; a view at byte offset 3: the aligned path refused),
its whole-wave path 192 finished episodes in a block ("dense" streams against "sparse" ones), its early-out a step without episodes (every
stream has some).  The dock scan reads 8-byte words (N = 5: bytewise; 8, 12: one word + tail; 65: a second lane; 4097: a second block), the
route scan 4-byte words when N is a multiple of 4 (N = 4, 68, 4100) and bytes otherwise (3, 5, 67, 4097); the chunk forms read rows at
(r chunk + t) n_local, misaligned for n_local = 100, 65 and 4097; population replicas start at k N."""
from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest
import torch

import tracker_streams as ts
from conftest import GOLDEN, load_golden_config
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import curriculum as pc
from rl_brain_trainer_amd import finisher_tools as ft
from rl_brain_trainer_amd import route_config as rcfg
from rl_brain_trainer_amd import route_curriculum as rc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DOCK_CFG = "dock_workspace_handoff_noop_ft_12env_raw"
SEEDS = [7, 8, 9]


# --------------------------------------------------------------------------------------------------------------------- helpers
def _dev(a: np.ndarray, offset: int = 0) -> torch.Tensor:
    """the bytes on the device, contiguous; offset > 0: as a view that many bytes into a larger buffer"""
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    if offset == 0:
        return flat.to(DEV)
    buf = torch.zeros(flat.numel() + 64, dtype=torch.uint8, device=DEV)
    view = buf[offset:offset + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    return view


def _window(st, ring) -> list[int]:
    n, head, cap = int(st.ring_len), int(st.ring_head), int(st.window_episodes)
    a = np.ctypeslib.as_array(ring)
    return [int(a[(head + j) % cap]) for j in range(n)]


def _snapshot(st, route: bool = False) -> dict:
    window = [_window(st, st.ring[q]) for q in range(4)] if route else _window(st, st.ring)
    assert int(st.ring_len) <= int(st.window_episodes) and 0 <= int(st.ring_head) < int(st.window_episodes)
    return {"stage": int(st.stage_index), "count": int(st.stage_episode_count), "window": window, "clock": int(st.num_timesteps), "n_events": int(st.n_events)}


def _frozen(st) -> bytes:
    """the tracker's bytes with the clock taken out"""
    copy = type(st).from_buffer_copy(bytes(st))
    copy.num_timesteps = 0
    return bytes(copy)


def _steps(spec: dict):
    route = spec["tracker"] == "route"
    return [(ts.done_bytes(spec, t), ts.flag_planes(spec, t) if route else None) for t in range(spec["T"])]


def _calls(spec: dict):
    """(first step, number of steps) of every device call: one step per call, or chunk_steps for a chunk stream"""
    chunk = spec["chunk"][1] if "chunk" in spec else 1
    assert spec["T"] % chunk == 0
    return [(t0, chunk) for t0 in range(0, spec["T"], chunk)]


def _check_point_history(st, events: list[dict]) -> None:
    assert int(st.n_events) == len(events)
    stored = min(len(events), pc.MAX_HISTORY)
    for k in range(stored):
        e, w = st.events[k], events[k]
        assert (e.from_stage, e.to_stage, e.trigger_success_rate, e.total_timesteps) == (w["from"], w["to"], w["rate"], w["total_timesteps"]), k


def _check_dock_history(st, events: list[dict]) -> None:
    assert int(st.n_events) == len(events)
    for k in range(min(len(events), ft.MAX_HISTORY)):
        e, w = st.events[k], events[k]
        assert (e.from_stage, e.to_stage, e.trigger_success_rate, e.stage_episode_count, e.total_timesteps) == \
               (w["from"], w["to"], w["rate"], w["stage_episode_count"], w["total_timesteps"]), k


def _check_route_history(st, events: list[dict]) -> None:
    assert int(st.n_events) == len(events)
    for k in range(min(len(events), rc.MAX_HISTORY)):
        e, w = st.events[k], events[k]
        assert (e.from_stage, e.to_stage, e.from_prefix_end_index, e.to_prefix_end_index, e.total_timesteps) == \
               (w["from"], w["to"], w["from_prefix"], w["to_prefix"], w["total_timesteps"]), k
        assert [e.recent_success_rate, e.recent_route_ready_hit_rate, e.recent_orientation_hit_rate, e.recent_regression_rate] == w["rates"], k


def _int32_at(ptr: int) -> int:
    from rl_brain_trainer_amd.vec_env import _view

    return int(_view(ptr, (1,), "<i4", DEV).cpu()[0])


# --------------------------------------------------------------------------------------------------------------------- point tracker
def _point(spec: dict) -> pc.PointCurriculum:
    p = spec["params"]
    return pc.PointCurriculum(success_rate_threshold=p["threshold"], window_episodes=p["window"], min_episodes_per_stage=p["min_episodes"],
                              max_stage_index=p["max_stage"], initial_stage_index=p["initial_stage"], device=0)


POINT_OBSERVE = [(f"point_{kind}_{n}", 0) for n in (1, 63, 64, 65, 4095, 4096, 4097, 8200) for kind in ("dense", "sparse")] + \
                [("point_mid_8200", 0), ("point_quiet_4097", 0), ("point_dense_4096", 3), ("point_sparse_4097", 3), ("point_dense_65", 3)]


@pytest.mark.parametrize("name,offset", POINT_OBSERVE, ids=[f"{n}+{o}" for n, o in POINT_OBSERVE])
def test_point_observe(name, offset):
    spec = ts.fixture()[name]["spec"]
    snaps, events = ts.replay_named(name)
    cur = _point(spec)
    before = _frozen(cur.read())
    idle_steps = 0
    for t, (done, _) in enumerate(_steps(spec)):
        cur.observe(_dev(done, offset), spec["N"])
        st = cur.read()
        assert _snapshot(st) == snaps[t], t
        assert _int32_at(cur.stage_ptr) == snaps[t]["stage"], t
        if not (done & 3).any():                                           # the early-out: only the clock moved
            idle_steps += 1
            assert _frozen(st) == before, t
        before = _frozen(st)
    assert idle_steps >= 1
    _check_point_history(cur.read(), events)
    if "quiet" in name:
        assert idle_steps == spec["T"] and events == []
    cur.close()


POINT_CHUNK = ["point_chunk_64_4_2", "point_chunk_100_3_3", "point_chunk_4097_2_2", "point_chunk_40_16_1"]


@pytest.mark.parametrize("name", POINT_CHUNK)
def test_point_observe_chunk(name):
    """rows at (r chunk + t) n_local of the rank-major block; the clock advances by world n_local per env step, not per rank"""
    spec = ts.fixture()[name]["spec"]
    n_local, chunk, world = spec["chunk"]
    snaps, events = ts.replay_named(name)
    steps = _steps(spec)
    cur = _point(spec)
    for t0, k in _calls(spec):
        block = ts.rank_blocks(np.stack([steps[t][0] for t in range(t0, t0 + k)]), world)
        cur.observe_chunk(_dev(block), n_local, chunk, world)
        st = cur.read()
        assert _snapshot(st) == snaps[t0 + k - 1], t0
        assert _int32_at(cur.stage_ptr) == snaps[t0 + k - 1]["stage"], t0
    _check_point_history(cur.read(), events)
    assert events and {e["total_timesteps"] % (n_local * world) for e in events} == {0}
    cur.close()


@pytest.mark.parametrize("n", [65, 4096])
def test_point_population(n):
    """three replicas on distinct streams and starting stages, one launch per step; the early-out is per replica: one replica never sees an
    episode (its bytes never change but for the clock) while the others promote"""
    names = [f"point_pop_{n}_a", f"point_pop_{n}_b", f"point_quiet_{n}"]
    specs = [ts.fixture()[k]["spec"] for k in names]
    shared = [{k: v for k, v in s["params"].items() if k != "initial_stage"} for s in specs]
    assert shared[0] == shared[1] == shared[2] and len({s["T"] for s in specs}) == 1
    p = specs[0]["params"]
    pop = pc.PointCurriculumPopulation(success_rate_threshold=p["threshold"], window_episodes=p["window"], min_episodes_per_stage=p["min_episodes"],
                                       max_stage_index=p["max_stage"], initial_stage_indices=[s["params"]["initial_stage"] for s in specs], device=0)
    replays = [ts.replay_named(k) for k in names]
    streams = [_steps(s) for s in specs]
    quiet_bytes = _frozen(pop.read(2))
    one_idle_while_another_promotes = False
    for t in range(specs[0]["T"]):
        pop.observe(_dev(ts.replica_major([streams[k][t][0] for k in range(3)])), n)
        for k in range(3):
            st = pop.read(k)
            assert _snapshot(st) == replays[k][0][t], (t, k)
            assert _int32_at(pop.device_state + k * C.sizeof(pc.CurriculumState)) == replays[k][0][t]["stage"], (t, k)
        assert _frozen(pop.read(2)) == quiet_bytes, t
        grew = [replays[k][0][t]["n_events"] > (replays[k][0][t - 1]["n_events"] if t else 0) for k in range(2)]
        idle = [not (streams[k][t][0] & 3).any() for k in range(2)]
        one_idle_while_another_promotes |= (grew[0] and idle[1]) or (grew[1] and idle[0])
    assert one_idle_while_another_promotes
    for k in range(3):
        _check_point_history(pop.read(k), replays[k][1])
    pop.close()


# --------------------------------------------------------------------------------------------------------------------- dock reverse tracker
def _dock_table(spec: dict):
    ref = ft.DockReverseCurriculum(stages=spec["params"]["stages"], window_episodes=spec["params"]["window"])
    return ref.resolved_stages(load_golden_config(DOCK_CFG))


def _assert_applied(config, record, where) -> None:
    """the config mirror holds the stage record's values (what read() copies out of the stage the device applied)"""
    c = config.c
    for key in ft._STAGE_ENV_KEYS:
        assert float(getattr(c.env, key)) == float(getattr(record, key)), (where, key)
    for key in ft._STAGE_RESET_SCALARS:
        assert float(getattr(c.dock_reset, key)) == float(getattr(record, key)), (where, key)
    for key in ft._STAGE_RESET_VECTORS:
        assert list(getattr(c.dock_reset, key)[:]) == list(getattr(record, key)[:]), (where, key)


def _dock_single(name: str, offset: int, real: str = "f32") -> None:
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    spec = ts.fixture()[name]["spec"]
    n_local, chunk, world = spec.get("chunk", (spec["N"], 1, 1))
    snaps, events = ts.replay_named(name)
    steps = _steps(spec)
    table = _dock_table(spec)
    assert len({(t.dock_residual_action_limit, t.close_bucket_probability) for t in table}) == len(table)     # every stage tells
    env = ArmKinematicVecEnv(load_golden_config(DOCK_CFG), 8, seed=3, real=real)       # the tracker takes n_local per call: any N on an 8-env handle
    cb = ft.DockReverseCurriculum(stages=spec["params"]["stages"], window_episodes=spec["params"]["window"])
    cb.attach(env)
    before = _frozen(cb.read())
    for t0, k in _calls(spec):
        rows = np.stack([steps[t][0] for t in range(t0, t0 + k)])
        if "chunk" in spec:
            cb.observe_chunk(_dev(ts.rank_blocks(rows, world), offset), n_local, chunk, world)
        else:
            cb.observe(_dev(rows[0], offset), spec["N"])
        st = cb.read()
        assert _snapshot(st) == snaps[t0 + k - 1], t0
        _assert_applied(env.config, table[snaps[t0 + k - 1]["stage"]], t0)
        if "quiet" in name:
            assert _frozen(st) == before, t0
    _check_dock_history(cb.read(), events)
    env.reset()                                                            # the handle still resets on the promoted stage
    assert torch.isfinite(env.info()["position_error_norm"]).all()
    cb.close()
    env.close()


DOCK_OBSERVE = [("dock_obs_5", 0), ("dock_obs_8", 0), ("dock_obs_12", 0), ("dock_obs_65", 0), ("dock_obs_4097", 0), ("dock_obs_12", 3), ("dock_obs_65", 3),
                ("dock_quiet_12", 0)]


@pytest.mark.parametrize("name,offset", DOCK_OBSERVE, ids=[f"{n}+{o}" for n, o in DOCK_OBSERVE])
def test_dock_observe(name, offset):
    _dock_single(name, offset)


@pytest.mark.parametrize("name", ["dock_chunk_12_4_2", "dock_chunk_65_3_3", "dock_chunk_4097_2_2"])
def test_dock_observe_chunk(name):
    """world > 1 and chunk_steps > 1: step by step, rank by rank; the clock advances once per env step"""
    _dock_single(name, 0)


def test_dock_observe_f64_handle():
    """the tracker kernel's fp64 form (it writes a promotion into a DevCfg<double>): the same stream, the same records"""
    _dock_single("dock_obs_65", 0, real="f64")


@pytest.mark.parametrize("names", [("dock_pop_12_a", "dock_pop_12_b", "dock_quiet_12_long"), ("dock_pop_65_a", "dock_pop_65_b", "dock_pop_65_c")],
                         ids=["12", "65"])
def test_dock_population(names):
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    specs = [ts.fixture()[k]["spec"] for k in names]
    n, T = specs[0]["N"], specs[0]["T"]
    assert all(s["params"] == specs[0]["params"] and (s["N"], s["T"]) == (n, T) for s in specs)
    replays = [ts.replay_named(k) for k in names]
    streams = [_steps(s) for s in specs]
    table = _dock_table(specs[0])
    env = ArmKinematicPopulationVecEnv(load_golden_config(DOCK_CFG), SEEDS, n, mode="dock")
    pcur = ft.DockReverseCurriculumPopulation(stages=specs[0]["params"]["stages"], window_episodes=specs[0]["params"]["window"], n_replicas=3)
    pcur.attach(env)
    raw = lambda obj: bytes(C.string_at(C.addressof(obj), C.sizeof(obj)))  # noqa: E731
    stages_seen = set()
    for t in range(T):
        pcur.observe(_dev(ts.replica_major([streams[k][t][0] for k in range(3)])), n)
        live = pcur.live_records()
        for k in range(3):
            st = pcur.read(k)
            want = replays[k][0][t]
            assert _snapshot(st) == want, (t, k)
            assert raw(live[k]) == raw(table[want["stage"]]), (t, k)
            _assert_applied(pcur.configs[k], table[want["stage"]], (t, k))
        stages_seen.add(tuple(replays[k][0][t]["stage"] for k in range(3)))
    assert any(len(set(s)) > 1 for s in stages_seen)                        # the replicas sat on different stages
    for k in range(3):
        _check_dock_history(pcur.read(k), replays[k][1])
    pcur.close()
    env.close()


# --------------------------------------------------------------------------------------------------------------------- route prefix tracker
def _route_cfg() -> dict:
    return json.loads((GOLDEN / "configs" / "route_curriculum_prefix120_routeobs_sequence2.json").read_text())


def _route_env(n: int):
    from rl_brain_trainer_amd.route_env import RouteVecEnv

    cfgd = _route_cfg()
    return RouteVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=120), rcfg.load_route_q(GOLDEN / "synthetic_route.json"), n, seed=2)


def _route_kw(spec: dict) -> dict:
    p = spec["params"]
    return dict(stages=rc.build_prefix_stages(p["prefixes"]), promotion_success_rate=p["success_rate"], promotion_route_ready_hit_rate=p["ready_rate"],
                promotion_orientation_hit_rate=p["orientation_rate"], promotion_max_regression_rate=p["max_regression_rate"],
                window_episodes=p["window"], min_episodes_per_stage=p["min_episodes"])


def _load_flags(views, flags: np.ndarray, rows=slice(None)) -> None:
    """the wrapper's flag planes as a step would have left them (route_ready, orientation hit, regression)"""
    for v, plane in zip(views, flags):
        v[rows].copy_(torch.from_numpy(plane).to(DEV))


def _flag_views(env):
    info = env.info()
    return [info["route_ready"], info["route_orientation_hit"], info["route_regression"]]


@pytest.mark.parametrize("name", ["route_obs_3", "route_obs_4", "route_obs_5", "route_obs_67", "route_obs_68", "route_obs_4097", "route_obs_4100", "route_quiet_5"])
def test_route_observe(name):
    spec = ts.fixture()[name]["spec"]
    prefixes = spec["params"]["prefixes"]
    snaps, events = ts.replay_named(name)
    env = _route_env(spec["N"])
    cb = rc.RoutePrefixCurriculumDevice(**_route_kw(spec))
    cb.attach(env)
    env.reset()
    views = _flag_views(env)
    before = _frozen(cb.read())
    for t, (done, flags) in enumerate(_steps(spec)):
        _load_flags(views, flags)
        cb.observe(_dev(done), spec["N"])
        st = cb.read()
        assert _snapshot(st, route=True) == snaps[t], t
        assert (env.route_cfg.reset.min_route_index, env.route_cfg.reset.max_route_index) == (1, prefixes[snaps[t]["stage"]]), t
        if "quiet" in name:
            assert _frozen(st) == before, t
    _check_route_history(cb.read(), events)
    env.reset()                                                            # the device config carries the promoted window
    assert 1 <= int(env.info()["route_index"].min()) and int(env.info()["route_index"].max()) <= prefixes[snaps[-1]["stage"]]
    cb.close()
    env.close()


@pytest.mark.parametrize("n", [1, 3, 5, 6, 7, 1023, 1024, 1025])
def test_route_episode_records(n):
    """(done & 0x0F) | ready << 4 | orientation hit << 5 | regression << 6 with the flags taken as != 0 (set bytes hold 1, 2, 0x80 or 0xFF): the word
    path (N a multiple of 4) and the bytewise one"""
    spec = {"seed": 400 + n, "N": n, "T": 12, "end_q16": [19661, 65536, 0], "succ": {"lo": 30000, "hi": 60000, "period": 50}, "flags_q16": [40000, 52000, 20000]}
    env = _route_env(n)
    cb = rc.RoutePrefixCurriculumDevice(stages=rc.build_prefix_stages([5, 10]), promotion_success_rate=0.75, promotion_route_ready_hit_rate=0.75,
                                        promotion_orientation_hit_rate=0.85, promotion_max_regression_rate=0.3, window_episodes=16, min_episodes_per_stage=24)
    cb.attach(env)
    env.reset()
    views = _flag_views(env)
    seen = set()
    for t in range(spec["T"]):
        done, flags = ts.done_bytes(spec, t), ts.flag_planes(spec, t)
        _load_flags(views, flags)
        out = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
        cb.record(_dev(done), out)
        assert out.cpu().numpy().tolist() == ts.record_bytes(done, flags).tolist(), t
        seen |= set(flags.reshape(-1).tolist())
    assert n < 8 or seen == {0, *ts.FLAG_SET_VALUES}
    cb.close()
    env.close()


@pytest.mark.parametrize("name", ["route_chunk_64_4_2", "route_chunk_100_3_3", "route_chunk_4097_2_2"])
def test_route_observe_chunk(name):
    """episode records of the helper in rank-major blocks (the 16-byte path needs an aligned run of 64 envs: n_local = 64 has it, 100 and 4097
    do not past row 0)"""
    spec = ts.fixture()[name]["spec"]
    n_local, chunk, world = spec["chunk"]
    prefixes = spec["params"]["prefixes"]
    snaps, events = ts.replay_named(name)
    records = [ts.record_bytes(done, flags) for done, flags in _steps(spec)]
    env = _route_env(8)
    cb = rc.RoutePrefixCurriculumDevice(**_route_kw(spec))
    cb.attach(env)
    for t0, k in _calls(spec):
        cb.observe_chunk(_dev(ts.rank_blocks(np.stack(records[t0:t0 + k]), world)), n_local, chunk, world)
        st = cb.read()
        assert _snapshot(st, route=True) == snaps[t0 + k - 1], t0
        assert env.route_cfg.reset.max_route_index == prefixes[snaps[t0 + k - 1]["stage"]], t0
    _check_route_history(cb.read(), events)
    env.reset()
    assert int(env.info()["route_index"].max()) <= prefixes[snaps[-1]["stage"]]
    cb.close()
    env.close()


def test_route_population():
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv

    names = ["route_pop_67_a", "route_pop_67_b", "route_pop_67_c"]
    specs = [ts.fixture()[k]["spec"] for k in names]
    n, T = specs[0]["N"], specs[0]["T"]
    assert all(s["params"] == specs[0]["params"] and (s["N"], s["T"]) == (n, T) for s in specs)
    prefixes = specs[0]["params"]["prefixes"]
    replays = [ts.replay_named(k) for k in names]
    streams = [_steps(s) for s in specs]
    cfgd = _route_cfg()
    env = RoutePopulationVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=120), rcfg.load_route_q(GOLDEN / "synthetic_route.json"),
                                SEEDS, n)
    pop = rc.RoutePrefixCurriculumPopulation(**_route_kw(specs[0]))
    pop.attach(env)
    env.reset()
    views = _flag_views(env)
    assert all(v.numel() == 3 * n for v in views)
    stages_seen = set()
    for t in range(T):
        for k in range(3):
            _load_flags(views, streams[k][t][1], slice(k * n, (k + 1) * n))
        pop.observe(_dev(ts.replica_major([streams[k][t][0] for k in range(3)])), n)
        for k in range(3):
            st = pop.read(k)
            assert _snapshot(st, route=True) == replays[k][0][t], (t, k)
            assert env.window(k) == (1, prefixes[replays[k][0][t]["stage"]]), (t, k)
        stages_seen.add(tuple(replays[k][0][t]["stage"] for k in range(3)))
    assert any(len(set(s)) > 1 for s in stages_seen)
    for k in range(3):
        _check_route_history(pop.read(k), replays[k][1])
    env.reset()
    index = env.info()["route_index"].cpu().numpy()
    for k in range(3):
        assert index[k * n:(k + 1) * n].max() <= prefixes[replays[k][0][-1]["stage"]], k
    pop.close()
    env.close()
