"""The population evaluator without a GPU: kp1_eval_step is exported, declared and bound with matching argument lists; what the library and
evaluate_workspace_expansion_population refuse is refused before any device work; the row / summary helper cuts a result table into
per-replica blocks."""
from __future__ import annotations

import ctypes as C
import json
import types

import numpy as np
import pytest

import abi
from conftest import GOLDEN, load_golden_config
from rl_brain_trainer_amd import evaluate as ev
from rl_brain_trainer_amd import native


def test_eval_step_symbol_exported_declared_and_bound():
    lib = C.CDLL(str(native.LIB_PATH))
    assert hasattr(lib, "kp1_eval_step")
    assert "kp1_eval_step" in native.declared_symbols()
    params = abi.params("kp1_eval_step", "kp1_ppo.h")
    L = native.load()
    assert len(L.kp1_eval_step.argtypes) == len(params) == 10
    for text, ctype in zip(params, L.kp1_eval_step.argtypes):
        if "*" in text and "kp1_eval_buffers" in text:
            assert ctype is C.POINTER(native.EvalBuffers), text
        elif "*" in text:
            assert ctype is C.c_void_p, text
        else:
            assert "int32_t" in text and ctype is C.c_int32, text


def test_eval_step_library_refusals_before_any_launch():
    """NULL handles, missing buffers and step < 1 are refused on the host with kp1_last_error text"""
    L = native.load()
    bufs = native.EvalBuffers()
    dummy = (C.c_uint8 * 64)()
    p = C.cast(dummy, C.c_void_p)
    assert L.kp1_eval_step(None, None, None, None, None, None, 1, None, 0, None) != native.KP1_OK
    assert b"NULL" in L.kp1_last_error()
    # non-NULL (never dereferenced) handles: the buffer and step checks come before the handles are looked at
    assert L.kp1_eval_step(p, p, p, p, p, C.byref(bufs), 1, None, 0, None) != native.KP1_OK
    assert b"NULL buffer" in L.kp1_last_error()
    full = native.EvalBuffers(*([p] * 9))
    assert L.kp1_eval_step(p, p, p, p, p, C.byref(full), 0, None, 0, None) != native.KP1_OK
    assert b"step 0" in L.kp1_last_error()
    part = native.EvalBuffers(p, p, p, p, p, None, None, None, p)
    assert L.kp1_eval_step(p, p, p, p, p, C.byref(part), 1, None, 0, None) != native.KP1_OK
    assert b"incomplete handoff buffers" in L.kp1_last_error()


def _fake_population(K=3, hidden=64, obs_dim=56):
    return types.SimpleNamespace(K=K, obs_dim=obs_dim, obs_w=64, cfg=types.SimpleNamespace(hidden=hidden), _mlp=None)


@pytest.mark.parametrize("pop,roots,match", [(_fake_population(K=3), ["a", "b"], "2 artifact roots for a population of 3"),
                                              (_fake_population(obs_dim=80), None, "route population"),
                                              (_fake_population(hidden=256), None, "hidden=256")])
def test_population_evaluator_host_refusals(pop, roots, match):
    """refused before any device call: this test runs without a GPU, and the suite (the first device call) is never built"""
    with pytest.raises(ValueError, match=match):
        ev.evaluate_workspace_expansion_population(population=pop, finisher_policy=None, approach_cfg=None, finisher_cfg=None, artifact_roots=roots)


def _table(n: int, seed: int) -> dict:
    """a hand-made result table of n episodes in the layout _eval_columns hands to the row / summary code"""
    g = np.random.default_rng(seed)
    A = {"final_position_error": g.uniform(0.0, 0.05, n), "final_orientation_error": g.uniform(0.0, 0.3, n),
         "final_action_magnitude": g.uniform(0.0, 0.5, n), "final_dq_norm": g.uniform(0.0, 0.02, n), "min_position_error": g.uniform(0.0, 0.01, n),
         "min_orientation_error": g.uniform(0.0, 0.05, n), "max_ready_streak": g.integers(0, 5, n).astype(np.int32)}
    F = {k: A[k] * 0.5 for k in ("final_position_error", "final_orientation_error", "final_action_magnitude", "final_dq_norm")}
    return {"A": A, "F": F, "success": g.random(n) < 0.7, "ready_hit": g.random(n) < 0.8, "ready_dwell": g.random(n) < 0.6,
            "position_regression": g.random(n) < 0.2, "orientation_regression": g.random(n) < 0.1}


def _cut(cols: dict, sl: slice) -> dict:
    return {k: ({kk: vv[sl] for kk, vv in v.items()} if isinstance(v, dict) else v[sl]) for k, v in cols.items()}


def test_row_summary_helper_on_a_table_cut_into_two_blocks(tmp_path):
    """the helper both evaluators call: each block's stage summaries are the plain means of its own rows, its selection is gated_score of
    those summaries (the function tests/golden/gated_score.json pins), and the three JSON files parse to the payload"""
    cfg = load_golden_config("approach_default")
    stages, episodes = [0, 2, 5], 4
    E = len(stages) * episodes
    table = _table(2 * E, 1)
    goal = np.random.default_rng(3).uniform(-1, 1, (E, 6))
    gate = {"score_stage_index": 2, "promotion_stage_success": 0.5}
    blocks = []
    for k in range(2):
        cols = _cut(table, slice(k * E, (k + 1) * E))
        payload = ev._workspace_payload(cols, goal, approach_cfg=cfg, stages=stages, episodes=episodes, seed=5, handoff_confirm_steps=2, gate_config=gate,
                                        artifact_root=tmp_path / f"b{k}")
        blocks.append(payload)
        assert payload["episodes_per_stage"] == episodes and payload["seed"] == 5 and len(payload["target_rows"]) == E
        for si, s in enumerate(stages):
            rows = [r for r in payload["target_rows"] if r["stage_index"] == s]
            assert [r["episode_id"] for r in rows] == list(range(episodes))
            sl = slice(si * episodes, (si + 1) * episodes)
            sm = payload["stage_metrics"][str(s)]
            assert sm["episode_count"] == episodes
            assert sm["success_rate"] == float(np.mean(cols["success"][sl])) and sm["finisher_ready_hit_rate"] == float(np.mean(cols["ready_hit"][sl]))
            assert sm["mean_final_position_error"] == float(np.mean([float(v) for v in cols["F"]["final_position_error"][sl]]))
            assert sm["mean_final_action_magnitude"] == float(np.mean([float(v) for v in cols["F"]["final_action_magnitude"][sl]]))
            assert sum(sm["failure_reason_counts"].values()) == episodes
            assert [r["goal_position"] for r in rows] == [goal[e][:3].tolist() for e in range(sl.start, sl.stop)]
        summaries = {int(k_): v for k_, v in payload["stage_metrics"].items()}
        assert payload["best_model_selection"] == ev.gated_score(summaries, 2, ev.gate_config_from_dict(gate))
        assert json.loads((tmp_path / f"b{k}" / "workspace_eval_summary.json").read_text()) == json.loads(json.dumps(payload))
        assert json.loads((tmp_path / f"b{k}" / "stage_metrics.json").read_text()) == json.loads(json.dumps(payload["stage_metrics"]))
        assert json.loads((tmp_path / f"b{k}" / "best_model_selection_summary.json").read_text()) == json.loads(json.dumps(payload["best_model_selection"]))
    assert blocks[0]["stage_metrics"] != blocks[1]["stage_metrics"]


def test_row_summary_helper_feeds_the_golden_gated_scores():
    """stage summaries in the helper's schema score as tests/golden/gated_score.json records (the selection half of a payload)"""
    cases = json.loads((GOLDEN / "gated_score.json").read_text())["cases"]
    assert cases
    for case in cases[:8]:
        sm = {int(k): v for k, v in case["stage_metrics"].items()}
        got = ev.gated_score(sm, int(case["score_stage_index"]), ev.gate_config_from_dict(case["gate"]))
        assert got.keys() == case["selection"].keys()
        for key, want in case["selection"].items():
            assert got[key] == pytest.approx(want, rel=1e-12, abs=1e-12), key
