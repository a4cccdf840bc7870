"""Chained sequential route evaluation on the device (kp1_route_chain_*, evaluate_sequential_route_batch, the teacher recorder and
`train_route --seeds`) against the shipped host-driven evaluator: every row field, summary, chunk metric, final q and artifact file of a
chain is `==` to evaluate_sequential_route with InferencePolicy.predict on the same weights.

Policies are built by hand so that outcomes are mixed.  The "servo net" copies eps * route_q_error (observation columns 47..53, the joint
error over the per-step joint limit, clipped to [-1, 1]) into seven hidden units -- eps = 0.01 keeps tanh in its linear region -- passes
them through layer 2 and scales back in the action head, so its action is g * route_q_error up to the tanh's cubic term.  With gain 0.6
it reaches every waypoint in 16 steps; with gain 0.4 it falls a little further behind at every waypoint and runs into the 24-step time limit
from the tenth waypoint on; the third policy is a seeded random net with the head scaled
until the clamp is met.  The fixture asserts on the REFERENCE rows that both outcomes occur."""
from __future__ import annotations

import ctypes as C
import functools
import json
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import route_config as rcfg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EPS = 0.01
SERVO_GAIN, SLOW_GAIN, RANDOM_HEAD_SCALE = 0.6, 0.4, 40.0
END = 12
FILES = ("route_eval_sequential_summary.json", "route_chunk_metrics.json", "route_eval_sequential_steps.jsonl", "route_failure_report.json")


@functools.lru_cache(maxsize=None)
def ref_root() -> Path:
    """where the shipped evaluator's artifact files of this session go"""
    return Path(tempfile.mkdtemp(prefix="route_chain_ref_"))


def chain_cfg() -> dict:
    cfgd = json.loads((GOLDEN / "configs" / "route_curriculum_prefix120_routeobs_sequence2.json").read_text())
    cfgd["env"]["termination"]["max_episode_steps"] = 24
    return cfgd


@functools.lru_cache(maxsize=None)
def route_q() -> np.ndarray:
    return rcfg.load_route_q(GOLDEN / "synthetic_route.json")


def servo_net(hidden: int, gain: float):
    from rl_brain_trainer_amd.ppo import ActorCritic

    ac = ActorCritic(hidden, DEV, seed=0, obs_dim=80)
    ac.flat.zero_()
    for j in range(7):
        ac.views["mlp_extractor.policy_net.0.weight"][j, 47 + j] = EPS
        ac.views["mlp_extractor.policy_net.2.weight"][j, j] = 1.0
        ac.views["action_net.weight"][j, j] = gain / EPS
    return ac


def random_net(hidden: int, seed: int, head_scale: float):
    from rl_brain_trainer_amd.ppo import ActorCritic

    ac = ActorCritic(hidden, DEV, seed=seed, obs_dim=80)
    ac.views["action_net.weight"].mul_(head_scale)
    return ac


@functools.lru_cache(maxsize=None)
def policies(hidden: int):
    return (servo_net(hidden, SERVO_GAIN), servo_net(hidden, SLOW_GAIN), random_net(hidden, 5, RANDOM_HEAD_SCALE))


@functools.lru_cache(maxsize=None)
def infer(hidden: int, p: int):
    from rl_brain_trainer_amd.ppo import InferencePolicy

    return InferencePolicy(policies(hidden)[p].state_dict(), device=DEV)


@functools.lru_cache(maxsize=None)
def reference(hidden: int, p: int, start: int, end: int) -> dict:
    """the shipped evaluator on policy p (computed once, shared, never modified)"""
    from rl_brain_trainer_amd.route_curriculum import evaluate_sequential_route

    return evaluate_sequential_route(policy=infer(hidden, p).predict, cfg=chain_cfg(), route_q=route_q(), start_index=start, end_index=end,
                                     artifact_root=ref_root() / f"ref_h{hidden}_p{p}_{start}_{end}")


def population_mlp(hidden: int, members: tuple[int, ...], max_batch: int = 8):
    from rl_brain_trainer_amd import mlp

    h = mlp.MlpKernels(hidden, DEV, max_batch=max_batch, obs_dim=80, replicas=len(members))
    h.pack(torch.stack([policies(hidden)[p].flat for p in members]).contiguous())
    return h


def assert_same_result(mine: dict, ref: dict, what) -> None:
    assert len(mine["rows"]) == len(ref["rows"]), what
    for a, b in zip(mine["rows"], ref["rows"]):
        assert list(a) == list(b), what
        for k in b:
            assert a[k] == b[k] and type(a[k]) is type(b[k]), (what, b["route_index"], k, a[k], b[k])
    for k in ref:
        assert mine[k] == ref[k], (what, k, mine[k], ref[k])


def assert_same_files(mine: Path, ref: Path, what) -> None:
    for name in FILES:
        assert (mine / name).read_bytes() == (ref / name).read_bytes(), (what, name)


def test_fixture_outcomes_are_mixed():
    """on the shipped evaluator's rows: the three policies together succeed somewhere and fail somewhere, and one of them fails after a success
    (what the stop-on-failure and recorder tests need)"""
    rows = [r for p in range(3) for r in reference(64, p, 1, END)["rows"]]
    print("reference outcomes:", [[int(r["success"]) for r in reference(64, p, 1, END)["rows"]] for p in range(3)])
    assert any(r["success"] for r in rows) and any(not r["success"] for r in rows)
    assert any(r["steps"] == 24 for r in rows), "no waypoint ran into the time limit"
    assert _failing_policy() is not None


def _failing_policy() -> int | None:
    """a policy whose chain 1..END succeeds at least once before its first failure"""
    for p in range(3):
        s = [r["success"] for r in reference(64, p, 1, END)["rows"]]
        if not all(s) and s[0]:
            return p
    return None


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("start", [1, 5])
def test_single_chain_equals_the_shipped_evaluator(tmp_path, hidden, start):
    from rl_brain_trainer_amd.route_curriculum import evaluate_sequential_route_batch

    ref = reference(hidden, 0, start, END)
    out = evaluate_sequential_route_batch(mlp=infer(hidden, 0)._mlp, cfg=chain_cfg(), route_q=route_q(), start_index=start, end_indices=[END],
                                          device=DEV, artifact_roots=[tmp_path / "chain"])
    assert len(out) == 1
    assert_same_result(out[0], ref, (hidden, start))
    assert_same_files(tmp_path / "chain", ref_root() / f"ref_h{hidden}_p0_{start}_{END}", (hidden, start))


@pytest.mark.parametrize("hidden", [64, 128])
def test_population_blocks_equal_single_results(hidden):
    from rl_brain_trainer_amd.route_curriculum import evaluate_sequential_route_batch

    ends = (12, 7, 1)
    pop = population_mlp(hidden, (0, 1, 2))
    out = evaluate_sequential_route_batch(mlp=pop, cfg=chain_cfg(), route_q=route_q(), start_index=1, end_indices=ends, device=DEV)
    pop.close()
    for k, e in enumerate(ends):
        assert_same_result(out[k], reference(hidden, k, 1, e), (hidden, k))


INFO_KEYS = ("position_error_norm", "orientation_error_norm", "route_q_error_norm", "route_ready", "route_ready_streak", "route_index",
             "action_l2", "executed_delta_q_l2", "q", "dq", "prev_action")


def _chain_env(n_rows: int, pitch: int):
    from rl_brain_trainer_amd.route_env import RouteVecEnv

    cfgd = chain_cfg()
    cfgd["route"]["sequence"]["enabled"] = False
    env = RouteVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=END), route_q(), n_rows, device=DEV, seed=0)
    env.set_obs_stride(pitch)
    return env


class _Lockstep:
    """one handle, one chain, one policy handle, stepped by hand"""

    def __init__(self, mlp_handle, n_rows: int, ends, stop_on_failure: bool = False) -> None:
        self.mlp = mlp_handle
        self.env = _chain_env(n_rows, 128)
        self.chain = self.env.chain(1, ends, stop_on_failure=stop_on_failure)
        self.obs = torch.zeros((n_rows, 128), device=DEV)
        self.act = torch.zeros((n_rows, 7), device=DEV)
        self.reward = torch.zeros(n_rows, device=DEV)
        self.done = torch.zeros(n_rows, dtype=torch.uint8, device=DEV)
        self.tags = torch.zeros((n_rows, 2), dtype=torch.int32, device=DEV)
        self.chain.begin(self.obs)

    def step(self) -> None:
        self.mlp.forward(self.obs, clipped=self.act)
        self.chain.step(self.act, self.obs, self.reward, self.done, self.tags)

    def close(self) -> None:
        self.chain.close()
        self.env.close()


def test_population_rows_track_single_handles_step_by_step():
    """K = 3 rows on one handle against three one-row handles: observations and info planes of alive rows after every lock step"""
    ends = (12, 7, 1)
    pop_mlp = population_mlp(64, (0, 1, 2))
    pop = _Lockstep(pop_mlp, 3, ends)
    singles = [_Lockstep(infer(64, k)._mlp, 1, [e]) for k, e in enumerate(ends)]
    rng0, base_rng0 = pop.env.rng_state().copy(), pop.env.base.rng_state().copy()
    assert torch.equal(pop.obs, torch.cat([s.obs for s in singles]))
    compared = 0
    for step in range(30):
        pop.step()
        for s in singles:
            s.step()
        info = pop.env.info()
        tags = pop.tags.cpu().numpy()
        for k, s in enumerate(singles):
            assert np.array_equal(tags[k], s.tags.cpu().numpy()[0]), (step, k)
            if tags[k][0] < 0:
                continue
            assert torch.equal(pop.obs[k], s.obs[0]) and torch.equal(pop.done[k], s.done[0]), (step, k)
            one = s.env.info()
            for key in INFO_KEYS:
                a, b = info[key], one[key]
                assert torch.equal(a[..., k], b[..., 0]), (step, k, key)
            compared += 1
    assert compared > 30 and int((tags[:, 0] < 0).sum()) >= 1      # the row to waypoint 1 has ended, the others were still compared
    # an explicit-state reset with a goal draws nothing: the wrapper's and the base env's streams stand where they started
    assert np.array_equal(pop.env.rng_state(), rng0) and np.array_equal(pop.env.base.rng_state(), base_rng0)
    pop.close()
    pop_mlp.close()
    for s in singles:
        s.close()


def test_two_rows_per_replica():
    """C = 2: six rows, per-row end indices (12, 5) inside each replica -- row r runs under replica r // 2's policy"""
    from rl_brain_trainer_amd.route_curriculum import evaluate_sequential_route_batch

    pop = population_mlp(64, (0, 1, 2))
    out = evaluate_sequential_route_batch(mlp=pop, cfg=chain_cfg(), route_q=route_q(), start_index=1, end_indices=[12, 5] * 3, rows_per_replica=2,
                                          device=DEV)
    pop.close()
    assert len(out) == 6
    for r in range(6):
        assert_same_result(out[r], reference(64, r // 2, 1, (12, 5)[r % 2]), r)
    assert out[0]["rows"] != out[2]["rows"] and out[2]["rows"] != out[4]["rows"]      # the replicas' policies differ


@pytest.mark.parametrize("p", [0, 1, 2])
def test_prefix_property(tmp_path, p):
    """the evaluation to end_index 5 is the first 5 rows of the evaluation to 12: what lets one chain per replica serve every gate prefix"""
    from rl_brain_trainer_amd.route_curriculum import evaluate_sequential_route_batch, sliced_evaluate

    ref5, ref12 = reference(64, p, 1, 5), reference(64, p, 1, END)
    assert ref12["rows"][:5] == ref5["rows"]
    out = evaluate_sequential_route_batch(mlp=infer(64, p)._mlp, cfg=chain_cfg(), route_q=route_q(), start_index=1, end_indices=[END], device=DEV)[0]
    assert out["rows"][:5] == ref5["rows"]
    env = _chain_env(1, 80)
    progress = env.route_progress_m.copy()
    env.close()
    sliced = sliced_evaluate(out["rows"], out["final_qs"], progress)(artifact_root=tmp_path / "s", start_index=1, end_index=5)
    assert sliced == {k: v for k, v in ref5.items() if k not in ("rows", "chunk_metrics", "final_q")}
    assert out["final_qs"][4] == ref5["final_q"]
    assert_same_files(tmp_path / "s", ref_root() / f"ref_h64_p{p}_1_5", p)


def test_stop_on_failure_ends_the_chain_at_the_first_failed_waypoint():
    from rl_brain_trainer_amd.route_curriculum import rows_from_chain_records

    p = _failing_policy()
    ref = reference(64, p, 1, END)["rows"]
    first_fail = next(i for i, r in enumerate(ref) if not r["success"])
    run = _Lockstep(infer(64, p)._mlp, 1, [END], stop_on_failure=True)
    tags = []
    total = sum(r["steps"] for r in ref[:first_fail + 1])
    for _ in range(total + 5):
        run.step()
        tags.append(run.tags.cpu().numpy()[0].copy())
    assert run.chain.alive() == 0
    rows = rows_from_chain_records(run.chain.records()[0], route_q(), 1)
    run.close()
    assert rows == ref[:first_fail + 1] and not rows[-1]["success"]
    tags = np.array(tags)
    want = [(r["route_index"], s) for r in ref[:first_fail + 1] for s in range(r["steps"])]
    assert [tuple(t) for t in tags[:total]] == want
    assert (tags[total:] == -1).all()


def test_recorder_cli_matches_a_host_loop(tmp_path):
    """collect_route_teacher on a saved servo-net checkpoint vs a Python loop over the single evaluator's env recording (obs, action) per step"""
    from rl_brain_trainer_amd import collect_route_teacher, teacher_anchor
    from rl_brain_trainer_amd.route_env import RouteVecEnv

    p = _failing_policy()
    ckpt = tmp_path / "teacher.pth"
    torch.save(policies(64)[p].state_dict(), ckpt)
    cfgd = chain_cfg()
    cfgd["route"].pop("init_checkpoint", None)
    cfg_path = tmp_path / "route.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgd))
    summary = collect_route_teacher.main(["--checkpoint", str(ckpt), "--config", str(cfg_path), "--route-path", str(GOLDEN / "synthetic_route.json"),
                                          "--artifact-root", str(tmp_path / "out"), "--start-index", "1", "--end-index", str(END)])
    # the host loop: the shipped evaluator's env and resets, recording before every step
    from rl_brain_trainer_amd.train_route import load_route_training_config

    cfg = load_route_training_config(cfg_path)
    seq_off = {**cfg, "route": {**cfg["route"], "sequence": {**cfg["route"]["sequence"], "enabled": False}}}
    env = RouteVecEnv(kcfg.to_env_config(cfg), rcfg.route_config_from_dict(seq_off, max_route_index=END), route_q(), 1, device=DEV, seed=0)
    pol = infer(64, p)
    cq, cdq, cpa = route_q()[0].copy(), np.zeros(7), np.zeros(7)
    obs_rows, act_rows, meta, good, bad = [], [], [], [], []
    for idx in range(1, END + 1):
        obs = env.reset(options={"route_index": idx, "start_route_index": 0, "initial_q": cq[None], "initial_dq": cdq[None],
                                 "initial_prev_action": cpa[None], "evaluator_state": True})
        first, done, steps = len(act_rows), 0, 0
        while not (done & 3):
            action = pol.predict(obs)
            obs_rows.append(obs[0].cpu().numpy().copy())
            act_rows.append(action[0].cpu().numpy().copy())
            meta.append((idx, steps))
            obs, _, d = env.step(action, auto_reset=False)
            done = int(d[0].item())
            steps += 1
        st = env.get_state()
        cq, cdq, cpa = st["q"][0].copy(), st["dq"][0].copy(), st["prev_action"][0].copy()
        if done & 4:
            good.append(idx)
        else:
            bad.append(idx)
            del obs_rows[first:], act_rows[first:], meta[first:]
            break
    env.close()
    assert good and bad, "the teacher must succeed somewhere and fail once"
    assert summary["successful_indices"] == good and summary["failed_indices"] == bad and summary["sample_count"] == len(act_rows)
    assert summary["schema_version"] == "v5.route_teacher_anchor_dataset.v1" and summary["action_dim"] == 7
    assert json.loads((tmp_path / "out" / "teacher_route_anchor_summary.json").read_text()) == summary
    flat = np.array(obs_rows, dtype=np.float32)
    with np.load(tmp_path / "out" / "teacher_route_anchor_dataset.npz") as data:
        assert np.array_equal(data["actions"], np.array(act_rows, dtype=np.float32)) and data["actions"].dtype == np.float32
        assert np.array_equal(data["route_index"], np.array([m[0] for m in meta], dtype=np.int32)) and data["route_index"].dtype == np.int32
        assert np.array_equal(data["step"], np.array([m[1] for m in meta], dtype=np.int32)) and data["step"].dtype == np.int32
        assert bad[0] not in set(data["route_index"].tolist())
        assert sorted(k[5:] for k in data.files if k.startswith("obs__")) == sorted(rcfg.ROUTE_OBS_LAYOUT) == summary["obs_keys"]
        for key, (off, width) in rcfg.ROUTE_OBS_LAYOUT.items():
            assert np.array_equal(data[f"obs__{key}"], flat[:, off:off + width]), key
    got_obs, got_act = teacher_anchor.load_anchor_dataset(tmp_path / "out" / "teacher_route_anchor_dataset.npz", END, 80)
    assert np.array_equal(got_obs, flat) and np.array_equal(got_act, np.array(act_rows, dtype=np.float32))
    # one imitation step on the recorded dataset runs
    from rl_brain_trainer_amd.ppo import PPO, PPOConfig

    env = RouteVecEnv(kcfg.to_env_config(cfg), rcfg.route_config_from_dict(cfg, max_route_index=END), route_q(), 16, device=DEV, seed=1)
    ppo = PPO(env, PPOConfig(n_steps=16, batch_size=64, n_epochs=1, hidden=64, seed=1), use_graphs=False)
    anchor = teacher_anchor.RouteTeacherAnchor(teacher_anchor.TeacherAnchorConfig(enabled=True, dataset_path=str(tmp_path / "out" / "teacher_route_anchor_dataset.npz"),
                                                                                  max_route_index=END))
    anchor.on_training_start(ppo)
    before = ppo.policy.flat.clone()
    loss = anchor.gradient_step(ppo, anchor._obs[:64], anchor._actions[:64])
    assert np.isfinite(loss) and not torch.equal(before, ppo.policy.flat)
    env.close()


def _normalised(path: Path, root: Path) -> str:
    return path.read_text().replace(str(root), "<root>")


def test_train_route_seeds_chained_evaluation_equals_per_replica_evaluation(tmp_path):
    from rl_brain_trainer_amd import checkpoint as ck
    from rl_brain_trainer_amd import train_route

    cfgd = chain_cfg()
    cfgd["route"]["curriculum"] = {**cfgd["route"].get("curriculum", {}), "prefix_stages": [4, 6], "promotion_window_episodes": 16,
                                   "min_episodes_per_stage": 16, "promotion_success_rate": 0.0, "promotion_route_ready_hit_rate": 0.0,
                                   "promotion_orientation_hit_rate": 0.0, "promotion_max_regression_rate": 1.0}
    cfgd["route"]["teacher_anchor"] = {"enabled": False}
    cfgd["route"]["sequential_gate"] = {"enabled": True, "prefixes": [3, 5], "full_end_index": 8}
    cfgd["route"]["route_path"] = str(GOLDEN / "synthetic_route.json")
    cfgd["route"].pop("init_checkpoint", None)
    cfg_path = tmp_path / "route.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgd))
    common = ["--config", str(cfg_path), "--n-envs", "16", "--n-steps", "64", "--batch-size", "256", "--hidden", "64", "--total-timesteps", "2048",
              "--seeds", "7,8", "--run-id", "t"]
    roots = {"chain": tmp_path / "chain", "host": tmp_path / "host"}
    train_route.main(common + ["--output-dir", str(roots["chain"])])
    train_route.main(common + ["--output-dir", str(roots["host"]), "--per-replica-eval"])
    compared = 0
    for s in (7, 8):
        a, b = roots["chain"] / f"seed_{s}", roots["host"] / f"seed_{s}"
        files = sorted(p.relative_to(b) for d in ("route_eval_sequential", "route_gate") for p in (b / d).rglob("*") if p.is_file())
        assert len(files) == 4 + 3 * 4 + 1, files     # the reached prefix, two gate prefixes and the full route, and the gate's verdict
        assert files == sorted(p.relative_to(a) for d in ("route_eval_sequential", "route_gate") for p in (a / d).rglob("*") if p.is_file())
        for f in files:
            assert _normalised(a / f, roots["chain"]) == _normalised(b / f, roots["host"]), (s, f)
            compared += 1
        accepted = [(r / "model_sequential_gate_accepted.zip").exists() for r in (a, b)]
        assert accepted[0] == accepted[1]
        if accepted[0]:
            sa, sb = (ck.load_policy_state_dict(r / "model_sequential_gate_accepted.zip") for r in (a, b))
            assert all(torch.equal(sa[k], sb[k]) for k in sb)
        ta, tb = (json.loads(_normalised(r / "training_summary.json", root)) for r, root in ((a, roots["chain"]), (b, roots["host"])))
        assert ta["evaluation_wall_seconds"] > 0 and tb["evaluation_wall_seconds"] > 0
        for key in ("route_eval_sequential_summary", "route_gate_summary", "curriculum_summary", "num_timesteps"):
            assert ta[key] == tb[key], (s, key)
        assert ta["route_gate_summary"]["full_result"]["end_index"] == 8
    assert compared == 34


def test_chain_refusals():
    """every refusal of the ABI: error text, no chain handle"""
    from rl_brain_trainer_amd.route_curriculum import RoutePrefixCurriculumDevice, build_prefix_stages
    from rl_brain_trainer_amd.route_env import RouteVecEnv

    cfgd = chain_cfg()
    off = json.loads(json.dumps(cfgd))
    off["route"]["sequence"]["enabled"] = False
    base = kcfg.to_env_config(cfgd)
    W = route_q().shape[0]

    def make(cfg_dict, n=2, **kw):
        return RouteVecEnv(base, rcfg.route_config_from_dict(cfg_dict, max_route_index=END), route_q(), n, device=DEV, seed=0, **kw)

    def refused(env, start, end, text, n_rows=None, exc=(ValueError, native.Kp1Error)):
        n = env.n_envs if n_rows is None else n_rows
        s = np.full(n, start, dtype=np.int32)
        e = np.full(n, end, dtype=np.int32)
        h = C.c_void_p()
        rc = env.L.kp1_route_chain_create(env._handle, C.c_void_p(s.ctypes.data), C.c_void_p(e.ctypes.data), n, 0, C.byref(h))
        assert rc != native.KP1_OK and not h.value
        assert text in env.L.kp1_last_error().decode(), env.L.kp1_last_error()
        with pytest.raises(exc):
            native.check(rc)

    env = make(off)
    L = env.L
    one = np.ones(2, dtype=np.int32)
    h = C.c_void_p()
    for args in ((None, C.c_void_p(one.ctypes.data), C.c_void_p(one.ctypes.data), 2, 0, C.byref(h)),
                 (env._handle, None, C.c_void_p(one.ctypes.data), 2, 0, C.byref(h)), (env._handle, C.c_void_p(one.ctypes.data), None, 2, 0, C.byref(h)),
                 (env._handle, C.c_void_p(one.ctypes.data), C.c_void_p(one.ctypes.data), 2, 0, None)):
        assert L.kp1_route_chain_create(*args) != native.KP1_OK and b"NULL" in L.kp1_last_error()
    refused(env, 0, 3, "start_index < 1")
    refused(env, 4, 3, "end_index < start_index")
    refused(env, 1, W, "end_index >= n_waypoints")
    refused(env, 1, 3, "env count", n_rows=3)
    chain = env.chain(1, 3)
    obs = torch.zeros((2, 80), device=DEV)
    assert L.kp1_route_chain_begin(env._handle, chain._h, None) != native.KP1_OK and b"NULL" in L.kp1_last_error()
    assert L.kp1_route_chain_step(env._handle, chain._h, None, C.c_void_p(obs.data_ptr()), None, None, None) != native.KP1_OK
    assert b"NULL" in L.kp1_last_error()
    # recorded reward components, switched on after the chain was made: refused at begin and at step
    env.enable_reward_components(True)
    assert L.kp1_route_chain_begin(env._handle, chain._h, C.c_void_p(obs.data_ptr())) != native.KP1_OK and b"reward components" in L.kp1_last_error()
    refused(env, 1, 3, "reward components")
    env.enable_reward_components(False)
    chain.close()
    # a prefix tracker attached to the handle
    cur = RoutePrefixCurriculumDevice(stages=build_prefix_stages([4, 6]), promotion_success_rate=0.8, promotion_route_ready_hit_rate=0.8,
                                      promotion_orientation_hit_rate=0.9, promotion_max_regression_rate=0.2, window_episodes=16)
    cur.attach(env)
    refused(env, 1, 3, "tracker")
    cur.close()
    env.chain(1, 3).close()       # and accepted again once the tracker is gone
    env.close()
    seq = make(cfgd)
    refused(seq, 1, 3, "sequence")
    seq.close()
    f64 = make(off, real="f64")
    refused(f64, 1, 3, "f32")
    f64.close()
