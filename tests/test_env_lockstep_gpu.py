"""The base env on the device in lockstep with the fp64 oracle: reward, every reward component, done bits, observations and counters of
200 envs on every step, both handles, every case of tests/golden/reward_fuzz.json plus the env-level fuzz configs and the shipped ones.

tests/env_lockstep.py holds the reference pass, the tie classification, the derivation of the tie widths and bounds, and the comparator;
tests/test_env_lockstep_cpu.py checks that side without a device.  f64 leg: strict, no ties (reward and components 1e-9, observations
6e-8, counters exact).  f32 leg: tie-tolerant, the existing constants for observations and pose errors, derived bounds for the weighted
components and the reward.
"""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

import env_lockstep as el
from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

pytestmark = pytest.mark.gpu

CHUNKS = el.chunks()
_refs: dict[str, el.Reference] = {}                 # the reference passes of the chunk in hand, shared by its two legs
_refs_chunk = [-1]
_reports: dict[tuple[str, str], tuple] = {}         # (real, case name) -> (mode, names, Report)


def _reference(chunk: int, index: int, case: el.Case) -> el.Reference:
    if _refs_chunk[0] != chunk:
        _refs.clear()
        _refs_chunk[0] = chunk
    if case.name not in _refs:
        _refs[case.name] = el.reference_pass(el.config_dict(case), case.stage, action_seed=index)
    return _refs[case.name]


def device_pass(R: el.Reference, real: str) -> tuple[dict, dict]:
    """the reference's action schedule on a device handle -> (reset0, per-step arrays) in the comparator's layout"""
    n, T = R.n, R.T
    env = ArmKinematicVecEnv(el.build_config(R.cfgd), n, seed=R.seed, real=real, reward_components=True)
    env.set_curriculum_stage(R.stage)
    env.reset()
    mask = torch.zeros(n, dtype=torch.uint8)
    mask[torch.as_tensor(R.limit_ids)] = 1
    obs0 = env.reset(options={"initial_q": R.limit_q, "goal_q": R.limit_goal_q}, mask=mask).cpu().numpy().copy()     # the limit group: masked reset with explicit options
    info = env.info()
    reset0 = {"obs": obs0, "rng": env.rng_state(), "q": env.get_state()["q"], "stage": info["stage_index"].cpu().numpy().astype(np.int64)}
    names, comps = env.reward_components()
    assert names == R.cls["names"]
    actions = torch.tensor(R.actions, dtype=env.dtype, device="cuda")
    keep = {k: [] for k in ("obs", "terminal_obs", "reward", "comps", "done", "dwell", "entry", "drift", "flags", "step_count", "stage", "q", "dq",
                            "ee", "pos_err", "ori_err", "entry_metrics")}
    src = {"dwell": "dwell_count", "entry": "near_goal_entry_count", "drift": "near_goal_drift_count", "flags": "flags", "step_count": "step_count",
           "stage": "stage_index", "pos_err": "position_error_norm", "ori_err": "orientation_error_norm"}
    rng = np.zeros((T, n, 6), np.uint64)
    q_exact = np.zeros((T, n, 7))
    for t in range(T):
        obs, rew, done = env.step(actions[t])
        for key, val in (("obs", obs), ("terminal_obs", env.terminal_obs), ("reward", rew), ("done", done), ("comps", comps.T)):
            keep[key].append(val.clone())
        for key, name in src.items():
            keep[key].append(info[name].clone())
        for key, name in (("q", "q"), ("dq", "dq"), ("ee", "ee_pose6"), ("entry_metrics", "entry_metrics")):
            keep[key].append(info[name].T.clone())
        if R.dev["rng_valid"][t]:
            rng[t] = env.rng_state()
            q_exact[t] = env.get_state()["q"]
    dev = {}
    for key, vals in keep.items():
        a = torch.stack(vals).cpu().numpy()
        dev[key] = a if key in ("obs", "terminal_obs") else (a.astype(np.float64) if a.dtype.kind == "f" else a.astype(np.int64))
    dev["rng"], dev["rng_valid"], dev["q_exact"] = rng, R.dev["rng_valid"].copy(), q_exact
    env.close()
    return reset0, dev


def _run(real: str, chunk: int, k: int, case: el.Case):
    if (real, case.name) not in _reports:
        index = sum(len(c) for c in CHUNKS[:chunk]) + k
        R = _reference(chunk, index, case)
        reset0, dev = device_pass(R, real)
        rep = el.compare(R, reset0, dev, strict=real == "f64", label=f"{case.name}[{real}]")
        print(f"\n[{case.name} {real}] {json.dumps(rep.summary())}")
        el.check_case_floors(R, rep)
        _reports[(real, case.name)] = (R.mode, R.cls["names"], rep, R.cfg)
    return _reports[(real, case.name)]


@pytest.mark.parametrize("real", ["f64", "f32"])
@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
def test_env_lockstep_vs_oracle(chunk, real):
    """Ten cases per test, N = 200 envs, max_episode_steps + 8 steps each (every env passes through the auto-reset inside the launch, the
    last 16 envs start next to a joint limit through reset(options=, mask=)).  Per case the comparator of tests/env_lockstep.py and the
    per-case caps and floors on what was compared.
    Observed on the MI355X: each test 0.3 - 1.2 s; the figures are in test_floors_and_worst_values_over_all_cases."""
    for k, case in enumerate(CHUNKS[chunk]):
        _run(real, chunk, k, case)


@pytest.mark.parametrize("real", ["f64", "f32"])
def test_floors_and_worst_values_over_all_cases(real):
    """Over all cases of one leg: every component of both modes non-zero on >= 50 compared, non-excused env-steps in >= 5 cases (this
    includes joint_limit_penalty, dock dq_penalty and delta_q_change_penalty, which no device test reached before), the dq clause of each
    readiness / low-motion gate seen with both values; prints the worst value and worst error / bound per quantity.
    Observed on the MI355X (profiles/r12_env_lockstep.json), worst over the 259 cases, 3.75 M env-steps per leg:
    f64: reward and components 1.4e-10 (0.14 of 1e-9; dock strict_center_position_penalty at 1.5e4), observations 5.96e-8 (one float32 ulp
    of the output), q / ee_pose6 / error norms <= 4.3e-14, every counter, done bit and RNG word equal, no env dropped.
    f32: no error above its bound; worst error / bound 0.65 for the weighted components (approach near_goal_bonus_scale, the powf of the
    decay, against the 16 * 2^-24 relative term), 0.41 for the reward, 0.60 for the raw-error components (5.97e-6, dock
    entry_to_curr_delta_action_l2 of fuzz4_dock, whose action limit is interpolated over the fp32 position error), observations 2.8e-6
    (0.14 of 2e-5), reset observations 2.4e-7, terminal observations 2.9e-6, position_error_norm 1.9e-7, orientation_error_norm 2.1e-6,
    ee_pose6 1.7e-6 and q 1.7e-6 (both fuzz0_approach, whose dynamic step scale lets q drift).  132 env-episodes state-tied over all cases
    (at most 6 of 200 in one case), 104 re-admitted at their reset; 51 698 of 51 800 first auto-resets compared; 1755 terminated-on-success
    episodes compared; 0.19 % of the env-step x component pairs excused; 6021 counter ties."""
    tot = el.Totals()
    worst: dict[str, float] = {}
    ratio: dict[str, tuple] = {}
    counts: dict[str, int] = {}
    for chunk, cases in enumerate(CHUNKS):
        for k, case in enumerate(cases):
            mode, names, rep, cfg = _run(real, chunk, k, case)
            R = el.Reference()
            R.mode, R.cls = mode, {"names": names}
            tot.add(R, rep)
            for key, v in rep.worst.items():
                worst[key] = max(worst.get(key, 0.0), v)
            for key, v in rep.ratio.items():
                if v >= ratio.get(key, (-1.0,))[0]:
                    ratio[key] = (v, str(rep.where.get(key)))
            for key, v in rep.counts.items():
                counts[key] = counts.get(key, 0) + v
    print("\nENV_LOCKSTEP_REPORT " + json.dumps({"real": real, "cases": len(el.all_cases()), "n_envs": el.N_ENVS,
                                                  "worst": {k: float(f"{v:.3g}") for k, v in sorted(worst.items())},
                                                  "worst_error_over_bound": {k: [float(f"{v[0]:.3g}"), v[1]] for k, v in sorted(ratio.items())},
                                                  "counts": counts}))
    assert tot.short() == [], tot.short()
