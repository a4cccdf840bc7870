"""The route env on the device in lockstep with the fp64 oracle under randomised route configs (tests/route_lockstep.py; the reference side is
checked without a device by tests/test_route_lockstep_cpu.py).

Every case of tests/golden/route_config_fuzz.npz on both handles through RouteVecEnv with recorded reward components: N = 200 envs (three
waves + 8 lanes: no multiple of the nearest kernel's 32 envs per block nor of 256), every env on every step for max_episode_steps + 8 = 48
steps, auto-reset inside the launch; the terminal observation is compared, then the fresh episode's reset state, RNG words and observation.
Both observation layouts (56 and 80 floats) occur; every seventh case runs at the padded pitch 64 / 128 (the pad must stay 0).
- f64: strict -- counters, flags, done bits, indices and RNG words exact, reward and components within 1e-9, observations within one float32
  ulp or 1e-9.
- f32: tie-tolerant, each quantity within its bound derived from the case's own config (route_lockstep.component_bounds).
A final test asserts the all-case floors on each handle's compared set and reports the worst error / bound per quantity.

Two more consumers of the same kernel text: the one-launch rollout step (kp1_mlp_forward_route_step) bit for bit against the launch sequence
on four fuzz cases, and a RoutePopulationVecEnv whose replica windows include the end of the route.

Measured on the MI355X (profiles/route_lockstep.json): f64 -- all 393 600 env-steps compared, reward 3.0e-14, components 2.4e-14,
observations 2.9e-11.  f32 -- 392 923 env-steps compared, 21 of 8200 envs dropped, 0.016 % of the pairs excused; worst error / bound 0.65
(curr_ori_error, random09), 0.51 (orientation_regression_penalty, ready_q0), 0.50 (ee_orientation_progress, random18), 0.47
(curr_pos_error against the 1e-7 position term, route_end2: 9.4e-8), 0.45 (ee_position_progress, route_end2), reward 0.29, observations
0.09; every floor met with the counts of the reference side.  No defect found in the device text.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import route_lockstep as rl
from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv, RouteVecEnv

pytestmark = pytest.mark.gpu

CHUNKS = rl.chunks()
PADDED_EVERY = 7
_refs: dict[str, rl.Reference] = {}
_reports: dict[tuple[str, str], rl.Report] = {}

INFO_KEYS = {"route_ready": "route_ready", "waypoint_success": "route_waypoint_success", "route_regression": "route_regression",
             "orientation_hit": "route_orientation_hit", "route_index": "route_index", "ready_streak": "route_ready_streak",
             "completed_waypoints": "route_completed_waypoints", "start_route_index": "start_route_index", "last_route_index": "last_route_index",
             "reset_mode": "route_reset_mode", "q_error_norm": "route_q_error_norm", "nearest_route_q_distance": "nearest_route_q_distance"}


def _reference(case: rl.Case) -> rl.Reference:
    if case.name not in _refs:
        _refs[case.name] = rl.reference_pass(rl.config_dict(case), rl.route_of(case), action_seed=case.index)
    return _refs[case.name]


def _reset_state(env: RouteVecEnv, obs: np.ndarray) -> dict:
    info = env.info()
    return {"obs": obs, "q": env.get_state()["q"].copy(), "rng": env.rng_state(),
            **{k: info[INFO_KEYS[k]].cpu().numpy().astype(np.int64) for k in ("route_index", "start_route_index", "last_route_index", "reset_mode")}}


def device_pass(env: RouteVecEnv, actions: np.ndarray) -> tuple[dict, dict]:
    """the device on the reference's action schedule, laid out as route_lockstep.as_device lays the reference out"""
    od, pitch = env.obs_dim, env.obs_stride
    first = env.reset().cpu().numpy()
    assert first.shape[1] == pitch and not first[:, od:].any()
    reset0 = _reset_state(env, first[:, :od].copy())
    rec = {k: [] for k in rl.DEVICE_KEYS}
    for a in actions:
        o, r, d = env.step(torch.tensor(a, device="cuda"))
        o, term = o.cpu().numpy(), env.terminal_obs.cpu().numpy()
        assert not o[:, od:].any() and not term[:, od:].any()
        info = env.info()
        _, comps = env.reward_components()
        rec["obs"].append(o[:, :od].copy())
        rec["terminal_obs"].append(term[:, :od].copy())
        rec["reward"].append(r.cpu().numpy().astype(np.float64))
        rec["bits"].append(d.cpu().numpy().astype(np.int64))
        rec["comps"].append(comps.cpu().numpy().T.astype(np.float64))
        for key, name in INFO_KEYS.items():
            v = info[name].cpu().numpy()
            rec[key].append(v.astype(np.float64 if v.dtype.kind == "f" else np.int64))
        rec["rng"].append(env.rng_state())
        rec["q"].append(env.get_state()["q"].copy())
    return reset0, {k: np.array(v) for k, v in rec.items()}


def _report(case: rl.Case, real: str) -> rl.Report:
    if (case.name, real) not in _reports:
        R = _reference(case)
        base, rc = rl.build_configs(R.cfgd)
        env = RouteVecEnv(base, rc, R.route_q, R.n, seed=R.seed, real=real, reward_components=True)
        assert env.obs_dim == case.obs_dim and env.dtype == (torch.float64 if real == "f64" else torch.float32)
        if case.index % PADDED_EVERY == 3:
            env.set_obs_stride(64 if case.obs_dim == 56 else 128)
        reset0, dev = device_pass(env, R.actions)
        env.close()
        rep = rl.compare(R, reset0, dev, strict=real == "f64", label=f"{case.name}/{real}")
        if real == "f32":
            rl.check_case_caps(R, rep)
        _reports[(case.name, real)] = rep
    return _reports[(case.name, real)]


@pytest.mark.parametrize("real", ["f64", "f32"])
@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
def test_route_env_lockstep_vs_oracle(chunk, real):
    for case in CHUNKS[chunk]:
        rep = _report(case, real)
        c = rep.counts
        print(f"\n[{case.name}/{real}] compared {c['compared_env_steps']} of {c['env_steps']} env-steps, state-tied envs {c['state_tied_envs']}, dropped "
              f"{c['dropped_envs']}, hand-overs {c['handovers']}, worst error / bound {max(rep.worst.ratio.values()):.3g}")


@pytest.mark.parametrize("real", ["f64", "f32"])
def test_floors_on_the_compared_set(real):
    """Totals.FLOORS on what the device was actually compared on; every error / bound below 1 (compare raises otherwise).  With
    ROUTE_LOCKSTEP_PROFILE=<path> the per-handle record is merged into that JSON file."""
    tot = rl.Totals()
    record = {"cases": 0, "env_steps": 0, "compared_env_steps": 0, "dropped_envs": 0, "excused_pairs": 0, "pairs": 0, "worst_error": {}, "worst_error_over_bound": {}}
    for case in rl.all_cases():
        rep = _report(case, real)
        tot.add(rep)
        record["cases"] += 1
        for k in ("env_steps", "compared_env_steps", "dropped_envs", "excused_pairs", "pairs"):
            record[k] += rep.counts[k]
        for name, src in (("worst_error", rep.worst.v), ("worst_error_over_bound", rep.worst.ratio)):
            for key, v in src.items():
                if key not in record[name] or v > record[name][key]["value"]:
                    record[name][key] = {"value": float(f"{v:.3g}"), "case": case.name}
    record["excused_share"] = float(f"{record['excused_pairs'] / record['pairs']:.3g}")
    record["floors"] = {**tot.counts, "sole_failing_clause": tot.sole, "cases_with_component_nonzero": tot.cases_nonzero.tolist()}
    print(f"\n[{real}] " + json.dumps(record))
    assert tot.short() == [], tot.short()
    assert max(v["value"] for v in record["worst_error_over_bound"].values()) < 1.0
    path = os.environ.get("ROUTE_LOCKSTEP_PROFILE")
    if path:
        old = json.loads(open(path).read()) if os.path.exists(path) else {}
        old[real] = record
        with open(path, "w") as f:
            f.write(json.dumps(old, indent=1, sort_keys=True) + "\n")


# ============================================================================== the route population: one window at the end of the route
def test_route_population_windows_vs_oracle():
    """K = 3 replicas x 40 envs in one RoutePopulationVecEnv on the sequence-length-3 case route_end0, replica windows [1, 20], [100, 170] and
    [478, 483] (route_window_of at the last waypoint), against 120 oracle envs with their own windows.  The case's segment and replay windows
    lie in [478, 483] and cannot lie in three disjoint windows at once, so these two reset modes get ratio 0 here."""
    case = rl.case_named("route_end0")
    cfgd = rl.config_dict(case)
    assert cfgd["route"]["sequence"] == {**cfgd["route"]["sequence"], "enabled": True, "sequence_length": 3}
    cfgd["route"]["reset"].update(segment_reset_ratio=0.0, replay_reset_ratio=0.0)
    K, n = 3, 40
    windows = [(1, 20), (100, 170), (478, 483)]
    R = rl.reference_pass(cfgd, rl.route_of(case), n=K * n, action_seed=99, windows=[windows[i // n] for i in range(K * n)])
    base, rc = rl.build_configs(cfgd)
    env = RoutePopulationVecEnv(base, rc, R.route_q, [R.seed + k * n for k in range(K)], n, reward_components=True)
    for k, (lo, hi) in enumerate(windows):
        env.set_replica_window(k, min_route_index=lo, max_route_index=hi)
    reset0, dev = device_pass(env, R.actions)
    env.close()
    for k, (lo, hi) in enumerate(windows):
        idx = reset0["route_index"][k * n:(k + 1) * n]
        assert idx.min() >= lo and idx.max() <= hi, (k, idx.min(), idx.max())
    rep = rl.compare(R, reset0, dev, label="population")
    c = rep.counts
    print(f"\n[population] {json.dumps(rep.summary())}")
    assert c["dropped_envs"] <= K * n // 20 and c["compared_first_resets"] >= 0.9 * c["first_resets"] and c["first_resets"] >= 0.9 * K * n
    assert c["sequence_success_at_route_end"] >= 20 and c["sequence_success_cut_by_window"] >= 20 and c["handovers"] >= 50


# ============================================================================== the one-launch rollout step on fuzz cases
# (case, what it is chosen for, the count on the launch-sequence twin that must be positive)
FUSED_CASES = [("ready_action0", "dwell 3 and a carried streak", "carried"), ("ready_dq1", "dwell 3", "dwell"),
               ("route_end1", "the window at the end of the route", "route_end"), ("ready_ori1", "a success that does not terminate", "no_termination")]


@pytest.mark.parametrize("name,why,needed", FUSED_CASES)
def test_fused_route_rollout_step_on_fuzz_cases(name, why, needed):
    """kp1_mlp_forward_route_step against kp1_mlp_forward + kp1_route_step on a twin env, bit for bit on every output of every step, every
    info plane and both RNG streams.  The policy's actions are small (|a| ~ 0.05), so an env that a recovery reset puts on its waypoint is
    route-ready at once and dwells; the branch the case is chosen for is counted on the twin."""
    import test_route_rollout_step_gpu as rs

    case = rl.case_named(name)
    cfgd = rl.config_dict(case)
    n, od = 70, case.obs_dim
    pitch = 128 if od == 80 else 64
    base = rl.build_configs(cfgd)[0]
    dwell, seq = int(base.c.termination.success_dwell_steps), bool(cfgd["route"]["sequence"]["enabled"])
    envs = []
    for _ in range(2):
        b, rc = rl.build_configs(cfgd)
        env = RouteVecEnv(b, rc, rl.route_of(case), n, seed=31, real="f32")
        env.set_obs_stride(pitch)
        envs.append(env)
    mlp = rs._mlp(64, 1, od, seed=5)
    from rl_brain_trainer_amd.ppo import ActorCritic
    pol = ActorCritic(64, rs.DEV, seed=5, obs_dim=od)
    pol.views["action_net.weight"].mul_(0.05)
    pol.views["log_std"].fill_(-4.0)
    mlp.pack(pol.flat.contiguous())
    env_a, env_b = envs
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=rs.DEV)   # noqa: E731
    obs_a, obs_b = env_a.reset().clone(), env_b.reset().clone()
    assert torch.equal(obs_a, obs_b)
    gen = torch.Generator(device=rs.DEV).manual_seed(7)
    counts = {k: 0 for k in ("carried", "dwell", "route_end", "no_termination", "reset", "waypoint_success")}
    last = rl.route_of(case).shape[0] - 1
    for t in range(60):
        noise = torch.randn((n, 7), generator=gen, device=rs.DEV)
        a = {"value": z(n), "action": z(n, 7), "log_prob": z(n), "next_obs": z(n, pitch), "reward": z(n), "done": z(n, dt=torch.uint8),
             "terminal_obs": z(n, pitch)}
        b = {k: torch.zeros_like(v) for k, v in a.items()}
        clipped = z(n, 7)
        target = env_b.info()["route_index"].clone()
        mlp.forward_route_step(env_a, obs_a, noise=noise, value=a["value"], action=a["action"], log_prob=a["log_prob"], next_obs=a["next_obs"],
                               reward=a["reward"], done=a["done"], terminal_obs=a["terminal_obs"])
        mlp.forward(obs_b, noise=noise, value=b["value"], action=b["action"], clipped=clipped, log_prob=b["log_prob"])
        env_b.step_into(clipped, b["next_obs"], b["reward"], b["done"], b["terminal_obs"], True)
        for k in a:
            assert torch.equal(a[k], b[k]), (name, t, k)
        ia, ib = env_a.info(), env_b.info()
        for k in ib:
            assert torch.equal(ia[k], ib[k]), (name, t, k)
        done = b["done"]
        wp = ib["route_waypoint_success"].ne(0)
        term, succ = (done & rs.TERMINATED).ne(0), (done & rs.SUCCESS).ne(0)
        fin = (done & 3).ne(0)
        counts["waypoint_success"] += int(wp.sum())
        counts["dwell"] += int(wp.sum()) if dwell == 3 else 0
        counts["carried"] += int((wp & ~fin & ib["route_ready_streak"].gt(0)).sum()) if seq else 0
        counts["route_end"] += int((succ & target.eq(last)).sum())
        counts["no_termination"] += int((succ & ~term).sum())
        counts["reset"] += int(fin.sum())
        obs_a, obs_b = a["next_obs"], b["next_obs"]
    assert np.array_equal(env_a.rng_state(), env_b.rng_state()) and np.array_equal(env_a.base.rng_state(), env_b.base.rng_state())
    print(f"\n[{name}] {why}: {counts}")
    assert counts[needed] > 0 and counts["reset"] >= n, counts
    mlp.close()
    for env in envs:
        env.close()
