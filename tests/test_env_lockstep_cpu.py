"""The reference side of the base-env lockstep parity (tests/env_lockstep.py), checked where there is no device.

Caps and floors of every case tests/test_env_lockstep_gpu.py runs, on the oracle alone (the "device" is the reference pass rounded through
float32): at most N // 20 state-tied envs, the drift counter untainted through the first episode of >= 50 % of the envs, >= 90 % of the first
auto-resets compared, < 2 % of the env-step x component pairs excused, >= 20 terminated-on-success episodes where the config terminates on
success; over all cases every component of both modes non-zero on >= 50 compared, non-excused env-steps in >= 5 cases, and the dq clause of
each readiness / low-motion gate seen with both values under the same floor.
Measured: at most 6 of 200 envs state-tied (fuzz041_approach), at least 168 clean first episodes and at most 0.41 % of the pairs excused
(both fuzz075_approach); the rarest component is dock basin_inner_exit_penalty, 454 env-steps in 24 cases.

Then the comparator's teeth: it passes the reference's own pass rounded through float32 and fails on each injected defect.
"""
from __future__ import annotations

import copy

import numpy as np
import pytest

import env_lockstep as el

CHUNKS = el.chunks()
_stats: dict[str, tuple] = {}      # case name -> (mode, component names, non-zero counts, dq-clause counts), filled by the chunk tests


def _case_stats(index: int, case: el.Case):
    if case.name not in _stats:
        R = el.reference_pass(el.config_dict(case), case.stage, action_seed=index)
        reset0, dev = el.as_device(R)
        rep = el.compare(R, reset0, dev, label=case.name, bounds=False)
        el.check_case_floors(R, rep)
        _stats[case.name] = (R, rep.nonzero, rep.dq_clause, rep.counts)
        R.dev = R.pre = R.excused = R.qty = R.width = R.eps = R.errors = None      # keep the small parts only
    return _stats[case.name]


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
def test_reference_caps_and_floors(chunk):
    first = sum(len(c) for c in CHUNKS[:chunk])
    for k, case in enumerate(CHUNKS[chunk]):
        counts = _case_stats(first + k, case)[3]
        print(f"\n[{case.name}] excused {counts['excused_pairs']} of {counts['pairs']} pairs, state-tied envs {counts['state_tied_envs']}, "
              f"clean first episodes {counts['drift_clean_first_episodes']}, counter ties {counts['counter_ties']}")


def test_every_component_and_dq_clause_is_exercised():
    tot = el.Totals()
    for index, case in enumerate(el.all_cases()):
        R, nonzero, dq_clause, _ = _case_stats(index, case)
        rep = el.Report(len(nonzero))
        rep.nonzero, rep.dq_clause = nonzero, dq_clause
        tot.add(R, rep)
    assert tot.short() == [], tot.short()


# ============================================================================== the comparator has teeth
TEETH_CASES = {"approach": (0, 57), "dock": (130, 200)}
WEIGHT = {"approach": ("reward", "position_progress_weight"), "dock": ("dock_reward", "orientation_progress_weight")}
THRESHOLD = {"approach": ("reward", "near_goal_pos_threshold_m"), "dock": ("dock_reward", "tight_pose_pos_threshold_m")}


@pytest.fixture(scope="module", params=["approach", "dock"])
def passes(request):
    out = []
    for index in TEETH_CASES[request.param]:
        case = el.all_cases()[index]
        cfgd = el.config_dict(case)
        out.append((case, cfgd, el.reference_pass(cfgd, case.stage, action_seed=index)))
    return request.param, out


def _mutant(R: el.Reference, cfgd: dict, case: el.Case, block: str, key: str, change) -> tuple[dict, dict]:
    """the oracle under the config with ONE value changed, replaying the reference's action schedule, laid out as a device pass"""
    m = copy.deepcopy(cfgd)
    m["env"][block][key] = change(m["env"][block][key])
    M = el.reference_pass(m, case.stage, actions=R.actions, classify=False)
    return el.as_device(M)


def test_comparator_passes_the_reference_rounded_to_float32(passes):
    for case, _, R in passes[1]:
        rep = el.compare(R, *el.as_device(R), label=case.name)
        assert max(rep.ratio.values()) < 0.25, rep.summary()     # float32 output rounding alone stays far below every bound
        el.compare(R, *el.as_device(R, f32=False), strict=True, label=case.name)


@pytest.mark.parametrize("defect", ["weight", "threshold", "success_dwell_steps"])
def test_comparator_fails_on_one_changed_config_value(passes, defect):
    mode, items = passes
    for case, cfgd, R in items:
        block, key, change = {"weight": (*WEIGHT[mode], lambda v: v * 1.01), "threshold": (*THRESHOLD[mode], lambda v: v * 1.01),
                              "success_dwell_steps": ("termination", "success_dwell_steps", lambda v: v + 1)}[defect]
        assert cfgd["env"][block][key] != 0
        with pytest.raises(el.Mismatch):
            el.compare(R, *_mutant(R, cfgd, case, block, key, change), label=case.name)


def test_comparator_fails_on_swapped_components_and_swapped_envs(passes):
    mode, items = passes
    for case, _, R in items:
        idx = R.cls["idx"]
        a, b = idx["position_progress"], idx["orientation_progress"]
        reset0, dev = el.as_device(R)
        dev["comps"][..., [a, b]] = dev["comps"][..., [b, a]]
        with pytest.raises(el.Mismatch):
            el.compare(R, reset0, dev, label=case.name)
        reset0, dev = el.as_device(R)              # a lane indexing error: the rows of two envs of different waves change places
        for key in el.DEVICE_KEYS:
            if dev[key].ndim >= 2:
                dev[key][:, [3, 70]] = dev[key][:, [70, 3]]
        with pytest.raises(el.Mismatch):
            el.compare(R, reset0, dev, label=case.name)
