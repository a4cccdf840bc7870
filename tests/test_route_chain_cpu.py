"""The chained route evaluation without a GPU: the chain ABI is exported, declared and bound with matching argument lists; what
evaluate_sequential_route_batch refuses is refused before any device work; the slicing ``evaluate`` callable, the recorder's
post-processing and the observation unflatten run on synthetic numpy data."""
from __future__ import annotations

import ctypes as C
import json
import re
import types

import numpy as np
import pytest

import abi
from rl_brain_trainer_amd import collect_route_teacher as rec
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import route_config as rcfg
from rl_brain_trainer_amd import route_curriculum as rc
from rl_brain_trainer_amd import teacher_anchor

CHAIN_SYMBOLS = {"kp1_route_chain_create": 6, "kp1_route_chain_destroy": 2, "kp1_route_chain_begin": 3, "kp1_route_chain_step": 7,
                 "kp1_route_chain_get_view": 2}


def test_chain_symbols_exported_declared_and_bound():
    lib = C.CDLL(str(native.LIB_PATH))
    L = native.load()
    for name, n_args in CHAIN_SYMBOLS.items():
        assert hasattr(lib, name), name
        assert name in native.declared_symbols(), name
        params = abi.params(name, "kp1_route.h")
        assert len(getattr(L, name).argtypes) == len(params) == n_args, name
        for text, ctype in zip(params, getattr(L, name).argtypes):
            if "kp1_route_chain_view" in text:
                assert ctype is C.POINTER(native.RouteChainView), text
            elif "**" in text:
                assert ctype is C.POINTER(C.c_void_p), text
            elif "*" in text:
                assert ctype is C.c_void_p, text
            else:
                assert "int32_t" in text and ctype is C.c_int32, text


def test_chain_record_layout_matches_the_header():
    from rl_brain_trainer_amd.route_env import CHAIN_RECORD

    header = (native.PKG_DIR.parent / "include" / "kp1_route.h").read_text()
    body = re.search(r"typedef struct kp1_route_chain_record \{(.*?)\} kp1_route_chain_record;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == list(CHAIN_RECORD.names)
    assert CHAIN_RECORD.itemsize == 6 * 4 + 8 * 8 + 4 * 7 * 8


def test_chain_library_refuses_null_arguments_before_any_device_call():
    L = native.load()
    dummy = (C.c_int32 * 4)(1, 1, 1, 1)
    p = C.cast(dummy, C.c_void_p)
    h = C.c_void_p()
    assert L.kp1_route_chain_create(None, p, p, 1, 0, C.byref(h)) != native.KP1_OK and b"NULL" in L.kp1_last_error()
    assert L.kp1_route_chain_create(p, None, p, 1, 0, C.byref(h)) != native.KP1_OK and b"NULL" in L.kp1_last_error()
    assert L.kp1_route_chain_create(p, p, p, 1, 0, None) != native.KP1_OK and b"NULL" in L.kp1_last_error()
    assert L.kp1_route_chain_begin(None, None, None) != native.KP1_OK and b"NULL" in L.kp1_last_error()
    assert L.kp1_route_chain_step(None, None, None, None, None, None, None) != native.KP1_OK and b"NULL" in L.kp1_last_error()
    assert L.kp1_route_chain_get_view(None, None) != native.KP1_OK and b"NULL" in L.kp1_last_error()
    assert not h.value


def _fake_mlp(replicas=3, obs_dim=80):
    return types.SimpleNamespace(replicas=replicas, obs_dim=obs_dim, obs_pad=128, max_batch=8)


@pytest.mark.parametrize("kwargs,exc,match", [
    (dict(end_indices=[12, 7, 500]), ValueError, "end index out of range"),
    (dict(end_indices=[12, 0, 3]), ValueError, "end index out of range"),
    (dict(end_indices=[12, 7, 3], start_index=0), ValueError, "start_index must be at least 1"),
    (dict(end_indices=[12, 7]), ValueError, "2 chains for a policy handle of 3 replicas"),
    (dict(end_indices=[12, 7, 3], rows_per_replica=2), ValueError, "expected 6"),
    (dict(end_indices=[12, 7, 3], artifact_roots=["a"]), ValueError, "1 artifact roots for 3 chains"),
    (dict(end_indices=[12, 7, 3], policy=lambda o: o), TypeError, "belong to evaluate_sequential_route"),
    (dict(end_indices=[12, 7, 3], real="f64", policy_needs_env=True), TypeError, r"\['policy_needs_env', 'real'\]"),
])
def test_batch_evaluator_host_refusals(kwargs, exc, match):
    """refused before any device call: this test runs without a GPU, and the env (the first device call) is never built.  The arguments of
    the single evaluator that have no meaning for packed policy handles (policy, policy_needs_env, real, ...) are named in the error."""
    route_q = np.zeros((20, 7))
    with pytest.raises(exc, match=match):
        rc.evaluate_sequential_route_batch(mlp=_fake_mlp(), cfg={"route": {}}, route_q=route_q, **kwargs)


def _rows(n: int, seed: int, start: int = 1) -> list[dict]:
    g = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        streak = int(g.integers(0, 3))
        rows.append({"route_index": start + i, "success": bool(g.random() < 0.7), "route_ready_hit": bool(g.random() < 0.8), "route_ready_dwell": streak >= 1,
                     "first_ready_step": int(g.integers(1, 20)) if streak else None, "max_ready_streak": streak, "steps": int(g.integers(1, 25)),
                     "final_position_error": float(g.uniform(0, 0.02)), "final_orientation_error": float(g.uniform(0, 0.3)),
                     "final_q_error": float(g.uniform(0, 0.6)), "min_position_error": float(g.uniform(0, 0.01)),
                     "min_orientation_error": float(g.uniform(0, 0.1)), "min_q_error": float(g.uniform(0, 0.1)),
                     "final_action_magnitude": float(g.uniform(0, 1.5)), "final_dq_norm": float(g.uniform(0, 0.05))})
    return rows


def test_sliced_evaluate_reproduces_the_summaries_of_the_slice(tmp_path):
    rows = _rows(50, 3)
    rows[0]["success"] = True
    final_qs = [[float(i)] * 7 for i in range(50)]
    progress = np.cumsum(np.full(60, 0.01))
    evaluate = rc.sliced_evaluate(rows, final_qs, progress)
    for end in (1, 7, 45, 50):
        got = evaluate(artifact_root=tmp_path / f"e{end}", start_index=1, end_index=end)
        want = rc.summarize_rows(rows[:end], progress)
        assert {k: got[k] for k in want} == want
        assert got["start_index"] == 1 and got["end_index"] == end and got["schema_version"] == "v5.route_curriculum.sequential_eval.v1"
        assert not {"rows", "chunk_metrics", "final_q"} & set(got)
        root = tmp_path / f"e{end}"
        assert json.loads((root / "route_eval_sequential_summary.json").read_text()) == json.loads(json.dumps(got))
        assert json.loads((root / "route_chunk_metrics.json").read_text()) == json.loads(json.dumps(rc.chunk_metrics(rows[:end])))
        lines = (root / "route_eval_sequential_steps.jsonl").read_text().splitlines()
        assert [json.loads(x) for x in lines] == rows[:end]
        report = json.loads((root / "route_failure_report.json").read_text())
        assert report["first_failure"] == next((r for r in rows[:end] if not r["success"]), None)
    assert len(rc.chunk_metrics(rows)) == 2 and len(rc.chunk_metrics(rows[:7])) == 1       # waypoints 1..40 and 41..50
    # the clamp of evaluate_sequential_route (an end past the route = the route's last waypoint) and what is not a slice of the chain
    assert rc.sliced_evaluate(rows, final_qs, progress[:51])(artifact_root=None, start_index=1, end_index=180)["end_index"] == 50
    with pytest.raises(ValueError, match="outside the chain"):
        evaluate(artifact_root=None, start_index=1, end_index=51)
    with pytest.raises(ValueError, match="not a slice"):
        evaluate(artifact_root=None, start_index=2, end_index=5)


def test_rows_from_chain_records_forms_the_start_error_on_the_host():
    from rl_brain_trainer_amd.route_env import CHAIN_RECORD

    g = np.random.default_rng(0)
    route_q = g.uniform(-1, 1, (6, 7))
    recs = np.zeros(2, dtype=CHAIN_RECORD)
    recs["route_index"] = [2, 3]
    recs["success"], recs["route_ready_hit"], recs["max_ready_streak"], recs["first_ready_step"], recs["steps"] = [1, 0], [1, 0], [2, 0], [4, -1], [5, 24]
    recs["min_q_error"] = [0.5, 1e-3]
    recs["start_q"][0] = route_q[2] + 0.01       # closer at the start than at any step
    recs["start_q"][1] = route_q[3] + 0.5
    rows = rc.rows_from_chain_records(recs, route_q, success_dwell_steps=2)
    assert rows[0]["min_q_error"] == float(np.linalg.norm(route_q[2] - recs["start_q"][0])) and rows[1]["min_q_error"] == 1e-3
    assert rows[0]["first_ready_step"] == 4 and rows[1]["first_ready_step"] is None
    assert rows[0]["route_ready_dwell"] is True and rows[1]["route_ready_dwell"] is False and rows[1]["success"] is False
    assert list(rows[0]) == ["route_index", "success", "route_ready_hit", "route_ready_dwell", "first_ready_step", "max_ready_streak", "steps",
                             "final_position_error", "final_orientation_error", "final_q_error", "min_position_error", "min_orientation_error",
                             "min_q_error", "final_action_magnitude", "final_dq_norm"]


def test_unflatten_is_the_inverse_of_flatten_observation():
    g = np.random.default_rng(1)
    for dim in (80, 56):
        flat = g.uniform(-1, 1, (9, dim)).astype(np.float32)
        keyed = rec.unflatten_observation(np.pad(flat, ((0, 0), (0, 128 - dim))), dim)       # padded policy rows: the padding is dropped
        assert sum(v.shape[1] for v in keyed.values()) == dim
        assert np.array_equal(teacher_anchor.flatten_observation(keyed, dim), flat)
    assert set(rec.unflatten_observation(np.zeros((1, 80), np.float32), 80)) == set(rcfg.ROUTE_OBS_LAYOUT)


def test_recorder_post_processing_drops_the_failed_waypoint(tmp_path):
    """tags + buffers -> dataset on synthetic arrays: two rows, row 0 fails at waypoint 3, row 1 succeeds at both of its waypoints"""
    g = np.random.default_rng(2)
    T, R = 12, 2
    tags = np.full((T, R, 2), -1, dtype=np.int32)
    plan = {0: [(1, 3), (2, 2), (3, 4)], 1: [(5, 6), (6, 5)]}
    for r, episodes in plan.items():
        t = 0
        for wp, steps in episodes:
            for s in range(steps):
                tags[t, r] = (wp, s)
                t += 1
    obs = g.uniform(-1, 1, (T, R, 128)).astype(np.float32)
    act = g.uniform(-1, 1, (T, R, 7)).astype(np.float32)
    arrays = rec.anchor_dataset_arrays(tags, obs, act, [{1, 2}, {5, 6}], 80)
    assert arrays["route_index"].tolist() == [1] * 3 + [2] * 2 + [5] * 6 + [6] * 5 and arrays["route_index"].dtype == np.int32
    assert arrays["step"].tolist() == [0, 1, 2, 0, 1] + list(range(6)) + list(range(5)) and arrays["step"].dtype == np.int32
    assert 3 not in arrays["route_index"]
    assert np.array_equal(arrays["actions"], np.concatenate([act[:5, 0], act[:11, 1]])) and arrays["actions"].dtype == np.float32
    np.savez_compressed(tmp_path / "d.npz", **arrays)
    flat, actions = teacher_anchor.load_anchor_dataset(tmp_path / "d.npz", 5, 80)       # the protected prefix: waypoints <= 5
    assert np.array_equal(flat, np.concatenate([obs[:5, 0, :80], obs[:6, 1, :80]])) and np.array_equal(actions, np.concatenate([act[:5, 0], act[:6, 1]]))
    empty = rec.anchor_dataset_arrays(tags, obs, act, [set(), set()], 80)
    assert empty["actions"].shape == (0, 7) and empty["obs__q"].shape == (0, 7)


def test_cli_flags():
    from rl_brain_trainer_amd import train_route

    args = train_route.build_arg_parser().parse_args(["--config", "c.yaml", "--seeds", "7,8", "--per-replica-eval"])
    assert args.per_replica_eval and not train_route.build_arg_parser().parse_args(["--config", "c.yaml"]).per_replica_eval
    a = rec.build_arg_parser().parse_args(["--checkpoint", "m.zip", "--config", "c.yaml", "--route-path", "r.json", "--artifact-root", "out"])
    assert (a.start_index, a.end_index) == (1, 120)
    cs = {"prefix_end_index": 20}
    assert train_route._chain_end_index({}, cs, 484) == 20
    assert train_route._chain_end_index({"sequential_gate": {"enabled": True, "full_end_index": 483}}, cs, 484) == 483
    assert train_route._chain_end_index({"sequential_gate": {"enabled": True}}, cs, 484) == 180
    assert train_route._chain_end_index({"sequential_gate": {"enabled": True, "prefixes": [3, 5], "full_end_index": 8}}, {"prefix_end_index": 6}, 13) == 8
    assert train_route._chain_end_index({"sequential_gate": {"enabled": True, "prefixes": [20, 40]}}, {"prefix_end_index": 6}, 13) == 12
