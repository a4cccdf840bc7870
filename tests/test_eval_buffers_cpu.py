"""evaluate.EpisodeBuffers without a GPU: the struct over the tensors, the layout include/kp1.h documents for kp1_eval_buffers, the meaning
results() gives every plane row, and the packing of the ready thresholds.  The expected mapping is written out here as a table; it is what
run_episodes and run_episodes_fused each spelled out before they shared the class."""
from __future__ import annotations

import ctypes as C
import types

import pytest
import torch

from rl_brain_trainer_amd import evaluate as ev
from rl_brain_trainer_amd import native

CPU = torch.device("cpu")
N = 3
FIELDS = [name for name, _ in native.EvalBuffers._fields_]
HAND_FIELDS = ("hand_metrics", "hand_step", "hand_success", "hand_state")
# field -> (shape, dtype) over N episodes, from the comments of kp1_eval_buffers in include/kp1.h
LAYOUT = {"metrics": ((8, N), torch.float64), "counters": ((4, N), torch.int32), "flags": ((4, N), torch.uint8), "state": ((N, 34), torch.float64),
          "hand_metrics": ((8, N), torch.float64), "hand_step": ((N,), torch.int32), "hand_success": ((N,), torch.uint8),
          "hand_state": ((N, 34), torch.float64), "n_alive": ((1,), torch.int32)}
# result key -> (plane, row, is a flag read as bool)
RES_ROWS = {"success": ("flags", 1, True), "final_position_error": ("metrics", 0, False), "final_orientation_error": ("metrics", 1, False),
            "min_position_error": ("metrics", 2, False), "min_orientation_error": ("metrics", 3, False), "final_action_magnitude": ("metrics", 4, False),
            "final_dq_norm": ("metrics", 5, False), "sum_action": ("metrics", 6, False), "sum_dq": ("metrics", 7, False),
            "ready_hit": ("flags", 2, True), "max_ready_streak": ("counters", 1, False), "first_ready_step": ("counters", 2, False),
            "step_count": ("counters", 0, False)}
HAND_ROWS = {"valid": ("flags", 3, True), "final_position_error": ("hand_metrics", 0, False), "final_orientation_error": ("hand_metrics", 1, False),
             "final_action_magnitude": ("hand_metrics", 2, False), "final_dq_norm": ("hand_metrics", 3, False),
             "min_position_error": ("hand_metrics", 4, False), "min_orientation_error": ("hand_metrics", 5, False)}
STATE_COLUMNS = {"state_q": (0, 7), "state_dq": (7, 14), "state_prev_action": (14, 21), "state_goal_q": (21, 28), "state_goal_pose6": (28, 34)}
STEP_COUNT = (0, 4, 4)          # episode 0 never stepped: its means divide by the clamped 1
HAND_STEP = (4, 0, 4)


@pytest.mark.parametrize("want_hand", [True, False])
def test_struct_holds_the_tensors_in_field_order(want_hand):
    b = ev.EpisodeBuffers(N, CPU, want_hand=want_hand)
    assert FIELDS == list(LAYOUT) == list(b.NAMES) and len(FIELDS) == 9
    for name in FIELDS:
        t = getattr(b, name)
        if name in HAND_FIELDS and not want_hand:
            assert t is None and not getattr(b.struct, name), name          # NULL in the struct
            continue
        assert getattr(b.struct, name) == t.data_ptr() != 0, name
        assert (tuple(t.shape), t.dtype) == LAYOUT[name] and t.is_contiguous() and t.device == CPU, name
    assert int(b.n_alive) == 0


def _filled(want_hand: bool) -> ev.EpisodeBuffers:
    """every plane holds values that name their own position: metrics[r, e] = 100 r + e, hand_metrics 1000 more, state[e, c] = 10000 + 100 e + c, ..."""
    b = ev.EpisodeBuffers(N, CPU, want_hand=want_hand)
    e = torch.arange(N)
    b.metrics.copy_(100.0 * torch.arange(8)[:, None] + e)
    b.counters.copy_(10 * torch.arange(4)[:, None] + e + 5)
    b.counters[0] = torch.tensor(STEP_COUNT)
    b.flags.copy_(torch.tensor([[1, 1, 1], [0, 1, 0], [1, 0, 0], [0, 0, 1]]))         # the four rows all differ
    b.state.copy_(10000.0 + 100.0 * e[:, None] + torch.arange(34))
    if want_hand:
        b.hand_metrics.copy_(1000.0 + 100.0 * torch.arange(8)[:, None] + e)
        b.hand_step.copy_(torch.tensor(HAND_STEP))
        b.hand_success.copy_(torch.tensor([1, 0, 1]))
        b.hand_state.copy_(20000.0 + 100.0 * e[:, None] + torch.arange(34))
    return b


def _assert_rows(out: dict, b: ev.EpisodeBuffers, rows: dict) -> None:
    for key, (plane, row, flag) in rows.items():
        want = getattr(b, plane)[row]
        assert torch.equal(out[key], want.bool() if flag else want) and out[key].dtype == (torch.bool if flag else want.dtype), key


def _assert_state(out: dict, plane: torch.Tensor) -> None:
    for key, (lo, hi) in STATE_COLUMNS.items():
        assert torch.equal(out[key], plane[:, lo:hi]) and out[key].shape == (N, hi - lo) and out[key].is_contiguous(), key


def test_results_map_every_plane_row_to_its_key():
    b = _filled(True)
    res, hand = b.results()
    assert set(res) == set(RES_ROWS) | {"mean_action_magnitude", "mean_dq_norm"} | set(STATE_COLUMNS)
    _assert_rows(res, b, RES_ROWS)
    steps = torch.tensor([1.0, 4.0, 4.0], dtype=torch.float64)             # STEP_COUNT with the 0 clamped to 1
    assert torch.equal(res["mean_action_magnitude"], b.metrics[6] / steps) and torch.equal(res["mean_dq_norm"], b.metrics[7] / steps)
    assert res["mean_action_magnitude"].tolist() == [600.0, 601.0 / 4, 602.0 / 4] and res["mean_dq_norm"].dtype == torch.float64
    _assert_state(res, b.state)

    assert set(hand) == set(HAND_ROWS) | {"step_count", "success", "mean_action_magnitude", "mean_dq_norm"} | set(STATE_COLUMNS)
    _assert_rows(hand, b, HAND_ROWS)
    assert torch.equal(hand["step_count"], b.hand_step) and hand["step_count"].dtype == torch.int32
    assert torch.equal(hand["success"], b.hand_success.bool()) and hand["success"].dtype == torch.bool
    hsteps = torch.tensor([4.0, 1.0, 4.0], dtype=torch.float64)            # HAND_STEP with the 0 clamped to 1
    assert torch.equal(hand["mean_action_magnitude"], b.hand_metrics[6] / hsteps) and torch.equal(hand["mean_dq_norm"], b.hand_metrics[7] / hsteps)
    assert hand["mean_dq_norm"].tolist() == [1700.0 / 4, 1701.0, 1702.0 / 4]
    _assert_state(hand, b.hand_state)


def test_results_without_handoff_buffers():
    b = _filled(False)
    res, hand = b.results()
    assert hand is None
    _assert_rows(res, b, RES_ROWS)
    _assert_state(res, b.state)


def test_thresholds_are_packed_in_the_order_pos_ori_action_dq():
    assert ev.EpisodeBuffers.thresholds(None) is None
    ready = types.SimpleNamespace(dock_coarse_ready_pos_threshold_m=0.25, dock_coarse_ready_ori_threshold_rad=0.5,
                                  dock_coarse_ready_action_threshold=2.0, dock_coarse_ready_dq_threshold=4.0,
                                  finisher_ready_pos_threshold_m=9.0)      # another predicate's field: not packed
    thr = ev.EpisodeBuffers(N, CPU, want_hand=False).thresholds(ready)
    assert len(thr) == 4 and thr._type_ is C.c_double and list(thr) == [0.25, 0.5, 2.0, 4.0]
