"""The reference side of the route-env lockstep parity (tests/route_lockstep.py), checked where there is no device.

Caps of every case tests/test_route_lockstep_gpu.py runs, on the oracle alone (the "device" is the reference pass rounded through float32):
at most N // 20 state-tied envs, >= 90 % of the first auto-resets compared, < 2 % of the env-step x component pairs excused.  Floors over
all cases (route_lockstep.Totals): every weighted component non-zero on >= 50 compared, non-excused env-steps in >= 5 cases; each clause of
route_ready the only failing one on >= 50 env-steps; >= 50 ready-but-not-reached steps, hand-overs with the streak carried and with it
cleared; >= 20 sequence successes at the last waypoint, sequence successes cut short by the window, successes that do not terminate, base
successes the wrapper suppresses, zero-tangent steps.
Measured: at most 7 of 200 envs state-tied (random02), at most 0.05 % of the pairs excused; the rarest floors are zero-tangent steps (893),
sequence successes at the last waypoint (931) and the orientation clause as the only failing one (7500); the rarest component is dq_penalty,
non-zero on >= 50 env-steps in 29 of the 41 cases.

The bounds at the four shipped configs stay below the constants the shipped-config tests used before.  Then the comparator's teeth: it
passes the reference's own pass rounded through float32 and fails on each injected defect.
"""
from __future__ import annotations

import copy

import numpy as np
import pytest

import route_lockstep as rl

CHUNKS = rl.chunks()
_reports: dict[str, rl.Report] = {}


def _report(case: rl.Case) -> rl.Report:
    if case.name not in _reports:
        R = rl.reference_pass(rl.config_dict(case), rl.route_of(case), action_seed=case.index)
        rep = rl.compare(R, *rl.as_device(R), label=case.name)
        rl.check_case_caps(R, rep)
        _reports[case.name] = rep
    return _reports[case.name]


def test_case_table_covers_what_the_shipped_configs_do_not():
    cases = [rl.config_dict(c) for c in rl.all_cases()]
    seq = [c["route"]["sequence"] for c in cases]
    term = [c["env"]["termination"] for c in cases]
    assert {s["sequence_length"] for s in seq if s["enabled"]} == {1, 2, 3, 4, 5}
    assert {s["reset_ready_streak_on_advance"] for s in seq if s["enabled"]} == {True, False} and {s["enabled"] for s in seq} == {True, False}
    assert {t["success_dwell_steps"] for t in term} == {1, 2, 3} and {t["terminate_on_success"] for t in term} == {True, False}
    assert {t["require_orientation"] for t in term} == {True, False} and {c["env"]["reward"]["use_orientation_gate"] for c in cases} == {True, False}
    assert {c.obs_dim for c in rl.all_cases()} == {56, 80}
    assert {(c["route"]["reset"]["min_route_index"], c["route"]["reset"]["max_route_index"]) for c in cases} >= {(1, 120), (1, 170), (478, 483), (478, 482)}
    for c in cases:
        r = c["route"]["reset"]
        assert r["replay_reset_ratio"] > 0 and r["recovery_reset_ratio"] > 0
        for key in ("segment_start_index", "segment_end_index", "replay_start_index", "replay_end_index"):
            assert r["min_route_index"] <= r[key] <= r["max_route_index"]
    weights = np.array([[v for k, v in sorted(c["route"]["reward"].items()) if "threshold" not in k] for c in cases])
    assert np.all((weights == 0.0).sum(axis=0) >= 1) and weights.max() > 8.5     # every weight is exactly 0 somewhere


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
def test_reference_caps(chunk):
    for case in CHUNKS[chunk]:
        c = _report(case).counts
        print(f"\n[{case.name}] state-tied envs {c['state_tied_envs']}, first resets {c['compared_first_resets']} of {c['first_resets']}, "
              f"excused {c['excused_pairs']} of {c['pairs']} pairs")


def test_floors_over_all_cases():
    tot = rl.Totals()
    for case in rl.all_cases():
        tot.add(_report(case))
    print("\n", tot.counts, tot.sole, tot.cases_nonzero.tolist())
    assert tot.short() == [], tot.short()


SHIPPED = [("route_curriculum_prefix120_routeobs_sequence2", 120), ("route_curriculum_prefix170_routeobs_sequence2", 170),
           ("route_curriculum_prefix20_sequence2", 20), ("route_curriculum_default", 20)]


@pytest.mark.parametrize("cfg_name,max_index", SHIPPED)
def test_bounds_at_the_shipped_configs_stay_below_the_old_constants(cfg_name, max_index):
    """component / reward / error / observation bounds evaluated on a reference pass of each shipped config <= COMP_TOL / REWARD_TOL /
    ERR_TOL / OBS_TOL of test_route_env_f32_gpu.py"""
    cfgd = rl.shipped_dict(cfg_name)
    cfgd["route"].setdefault("reset", {}).setdefault("max_route_index", max_index)
    R = rl.reference_pass(cfgd, rl.synthetic_route(), n=100, steps=60)
    flat = lambda x: x.reshape(-1, *x.shape[2:])
    b = rl.component_bounds(R.rc, flat(R.comps), flat(R.action_norm), flat(R.dq_norm), flat(R.a2), flat(R.da2), flat(R.q_error_norm),
                            flat(R.nearest_route_q_distance), flat(R.fresh))
    assert np.max(b["comps"]) <= rl.COMP_TOL and np.max(np.sum(b["comps"], axis=1)) <= rl.REWARD_TOL, (np.max(b["comps"], axis=0), np.max(np.sum(b["comps"], axis=1)))
    assert max(np.max(b["err"]), np.max(b["q_err"]), np.max(b["nearest"])) <= rl.ERR_TOL
    assert np.max(rl.obs_bounds(R.base, flat(R.step_obs))) <= rl.OBS_TOL
    assert int(R.waypoint_success.sum()) > 50 and int(R.done.sum()) > 50


# ============================================================================== the comparator has teeth
@pytest.fixture(scope="module")
def passes():
    """a sequence case with dwell > 1 and the streak carried, and the window that ends at the last waypoint"""
    out = {}
    for name in ("ready_action0", "route_end0", "random14"):
        case = rl.case_named(name)
        cfgd = rl.config_dict(case)
        out[name] = (case, cfgd, rl.reference_pass(cfgd, rl.route_of(case), action_seed=case.index))
    return out


def _mutant(R: rl.Reference, cfgd: dict, path: tuple, change) -> tuple[dict, dict]:
    """the oracle under the config with ONE value changed, replaying the reference's action schedule, laid out as a device pass"""
    m = copy.deepcopy(cfgd)
    node = m
    for key in path[:-1]:
        node = node[key]
    node[path[-1]] = change(node[path[-1]])
    return rl.as_device(rl.reference_pass(m, R.route_q, actions=R.actions))


def test_comparator_passes_the_reference_rounded_to_float32(passes):
    for case, _, R in passes.values():
        rep = rl.compare(R, *rl.as_device(R), label=case.name)
        assert max(rep.worst.ratio.values()) < 0.25, rep.summary()     # float32 output rounding alone stays far below every bound
        rl.compare(R, *rl.as_device(R, f32=False), strict=True, label=case.name)


def _reward_fields(R: rl.Reference, cfgd: dict, **values) -> tuple[dict, dict]:
    """as _mutant, with route.reward fields replaced by the NAMED fields' values (a kernel reading a threshold from the wrong field)"""
    m = copy.deepcopy(cfgd)
    for key, source in values.items():
        m["route"]["reward"][key] = cfgd["route"]["reward"][source]
    return rl.as_device(rl.reference_pass(m, R.route_q, actions=R.actions))


DEFECTS = {
    "weight": lambda c, R: _mutant(R, c, ("route", "reward", "ee_position_progress_weight"), lambda v: v * 1.01),
    "action_dq_thresholds_swapped": lambda c, R: _reward_fields(R, c, route_ready_action_threshold="route_ready_dq_threshold",
                                                                route_ready_dq_threshold="route_ready_action_threshold"),
    "q_threshold_from_pos_field": lambda c, R: _reward_fields(R, c, route_ready_q_threshold="route_ready_pos_threshold_m"),
    "dwell_plus_1": lambda c, R: _mutant(R, c, ("env", "termination", "success_dwell_steps"), lambda v: v + 1),
    "dwell_minus_1": lambda c, R: _mutant(R, c, ("env", "termination", "success_dwell_steps"), lambda v: v - 1),
    "sequence_length_plus_1": lambda c, R: _mutant(R, c, ("route", "sequence", "sequence_length"), lambda v: v + 1),
    "sequence_length_minus_1": lambda c, R: _mutant(R, c, ("route", "sequence", "sequence_length"), lambda v: v - 1),
    "streak_flag": lambda c, R: _mutant(R, c, ("route", "sequence", "reset_ready_streak_on_advance"), lambda v: not v),
    "terminate_on_success": lambda c, R: _mutant(R, c, ("env", "termination", "terminate_on_success"), lambda v: not v),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_comparator_fails_on_one_changed_config_value(passes, defect):
    # terminate_on_success only shows on the single-waypoint env (random14); the sequence settings on a sequence env
    name = "random14" if defect == "terminate_on_success" else "ready_action0"
    case, cfgd, R = passes[name]
    if defect.startswith("dwell_minus"):
        assert cfgd["env"]["termination"]["success_dwell_steps"] >= 2
    if defect.startswith("sequence_length_minus"):
        assert cfgd["route"]["sequence"]["sequence_length"] >= 2
    with pytest.raises(rl.Mismatch):
        rl.compare(R, *DEFECTS[defect](cfgd, R), label=case.name)


def test_comparator_fails_on_window_max_off_by_one_at_the_route_end(passes):
    case, cfgd, R = passes["route_end0"]
    assert cfgd["route"]["reset"]["max_route_index"] == rl.synthetic_route().shape[0] - 1
    with pytest.raises(rl.Mismatch):
        rl.compare(R, *_mutant(R, cfgd, ("route", "reset", "max_route_index"), lambda v: v - 1), label=case.name)


def test_comparator_fails_on_swapped_components_and_swapped_envs(passes):
    for case, _, R in passes.values():
        reset0, dev = rl.as_device(R)
        dev["comps"][..., [1, 2]] = dev["comps"][..., [2, 1]]
        with pytest.raises(rl.Mismatch):
            rl.compare(R, reset0, dev, label=case.name)
        reset0, dev = rl.as_device(R)              # a lane indexing error: the rows of two envs of different waves change places
        for key in rl.DEVICE_KEYS:
            dev[key][:, [3, 70]] = dev[key][:, [70, 3]]
        with pytest.raises(rl.Mismatch):
            rl.compare(R, reset0, dev, label=case.name)
