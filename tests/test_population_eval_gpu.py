"""The one-launch evaluation step (kp1_eval_step / eval_step_kernel) and the population evaluator built on it, on the GPU.

Shapes: E = 70 rows per replica (more than one row tile and a ragged last tile for a 32- or a 64-row tile), K = 3, weights of three
differently seeded ActorCritics with the action head scaled up so that part of the mean actions leave [-1, 1] and the clamp is exercised.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest
import torch

import eval_forms as F
from conftest import load_golden_config
from eval_forms import DEV, THR
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import evaluate as ev
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import ppo as P
from rl_brain_trainer_amd.mlp import MlpKernels
from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

pytestmark = pytest.mark.gpu
E, K = 70, 3


@pytest.fixture(scope="module")
def policies():
    """hidden -> the three K = 1 InferencePolicy of the three seeds (their MlpKernels are the K = 1 handles of the fused runs)"""
    return {h: [P.InferencePolicy(F.state_dict(h, 11 + k), device=DEV, max_batch=128) for k in range(K)] for h in (64, 128)}


@pytest.fixture(scope="module")
def suite():
    """70 explicit resets: 35 episodes each of two stages of approach_default's curriculum-local suite"""
    return F.build_suite(load_golden_config("approach_default"), E // 2)


def _opts(suite, mode: str, reps: int = 1) -> dict:
    return {**{k: np.tile(v, (reps, 1)) for k, v in suite.items()}, "policy_mode": mode}


def _cfg(mode: str):
    return load_golden_config("approach_default" if mode == "approach" else "dock_default")


def _fused_run(mlp: MlpKernels, mode: str, stride: int, opts: dict, n: int, confirm: int, active: torch.Tensor, on_step=None) -> tuple[ev.EpisodeBuffers, ArmKinematicVecEnv]:
    """episodes to the step limit through kp1_eval_step on the env's own buffers"""
    L = native.load()
    env = F.make_env(_cfg(mode), n, stride, opts)
    b = ev.EpisodeBuffers(n, DEV, want_hand=True)
    thr = (C.c_double * 4)(*THR)
    native.check(L.kp1_eval_accumulate(env._handle, C.byref(b.struct), None, None, F.ptr(active), 0, thr, confirm, F.stream()))
    for step in range(1, env.config.c.termination.max_episode_steps + 2):
        native.check(L.kp1_eval_step(mlp._h, env._handle, F.ptr(env.obs), F.ptr(env.reward), F.ptr(env.done), C.byref(b.struct), step, thr, confirm, F.stream()))
        if on_step is not None:
            on_step(step, env, b)
    return b, env


def _active_mask(n: int) -> torch.Tensor:
    m = torch.tensor(np.random.default_rng(2).random(n) < 0.85, device=DEV).to(torch.uint8).contiguous()
    assert 0 < int(m.sum()) < n
    return m


# ---------------------------------------------------------------------------------------------------------------- 1. step parity, K = 1
@pytest.mark.parametrize("confirm", [0, 2])
@pytest.mark.parametrize("stride", [56, 64])
@pytest.mark.parametrize("mode", ["approach", "dock"])
@pytest.mark.parametrize("hidden", [64, 128])
def test_eval_step_equals_the_launch_sequence(policies, suite, hidden, mode, stride, confirm):
    """kp1_eval_step against InferencePolicy.predict + the norm written out term by term + env.step(auto_reset=False) +
    kp1_eval_accumulate on a second handle: after EVERY step the observation buffer, the done bytes and every env.info() field, at the end
    every eval buffer, bit for bit."""
    L = native.load()
    pol = policies[hidden][0]
    opts = _opts(suite, mode)
    active = _active_mask(E)
    ref_env = F.make_env(_cfg(mode), E, stride, opts)
    rb = ev.EpisodeBuffers(E, DEV, want_hand=True)
    thr = (C.c_double * 4)(*THR)
    native.check(L.kp1_eval_accumulate(ref_env._handle, C.byref(rb.struct), None, None, F.ptr(active), 0, thr, confirm, F.stream()))
    clamped = {"lo": 0, "in": 0}

    def on_step(step, env, b):
        action = pol.predict(ref_env.obs)
        clamped["lo"] += int((action.abs() == 1.0).sum())
        clamped["in"] += int((action.abs() < 1.0).sum())
        an = F.norm_in_index_order(action)
        ref_env.step(action, auto_reset=False)
        native.check(L.kp1_eval_accumulate(ref_env._handle, C.byref(rb.struct), F.ptr(an), F.ptr(ref_env.done), None, step, thr, confirm,
                                           F.stream()))
        assert torch.equal(env.obs, ref_env.obs), ("obs", step)
        assert torch.equal(env.done, ref_env.done), ("done", step)
        fi, ri = env.info(), ref_env.info()
        for k in ri:
            assert torch.equal(fi[k], ri[k]), (k, step)
        assert torch.equal(b.n_alive, rb.n_alive), ("n_alive", step)

    b, env = _fused_run(pol._mlp, mode, stride, opts, E, confirm, active, on_step)
    for name in F.NAMES:
        assert torch.equal(getattr(b, name), getattr(rb, name)), name
    assert clamped["lo"] > 0 and clamped["in"] > 0                      # the clamp was met, and not everywhere
    assert int(rb.n_alive) == 0 and int(rb.counters[0].max()) >= 2       # episodes ran, and to their end
    assert bool((rb.flags[0] == 0).all()) and torch.equal(rb.counters[0][active == 0], torch.zeros_like(rb.counters[0][active == 0]))
    if confirm == 0:
        assert torch.equal(rb.flags[3], active)                          # ready_streak >= 0 hands over at step 1
    env.close()
    ref_env.close()


# ---------------------------------------------------------------------------------------------------------------- 2. population parity
@pytest.mark.parametrize("hidden", [64, 128])
def test_population_block_equals_single_fused_run(policies, suite, hidden):
    """block k of a K = 3 population handle over 3 x 70 envs == the K = 1 fused run of replica k's weights.  The population handle's
    max_batch (64) is smaller than the 70 rows per replica: the step uses no activation workspace."""
    pop = MlpKernels(hidden, DEV, max_batch=64, replicas=K)
    pop.pack(torch.stack([p.policy.flat for p in policies[hidden]]).contiguous())
    active = _active_mask(K * E)
    pb, penv = _fused_run(pop, "approach", 64, _opts(suite, "approach", K), K * E, 2, active)
    pinfo = {k: v.clone() for k, v in penv.info().items()}
    for k in range(K):
        sl = slice(k * E, (k + 1) * E)
        sb, senv = _fused_run(policies[hidden][k]._mlp, "approach", 64, _opts(suite, "approach"), E, 2, active[sl].contiguous())
        assert torch.equal(penv.obs[sl], senv.obs) and torch.equal(penv.done[sl], senv.done), k
        for name, v in senv.info().items():
            assert torch.equal(pinfo[name][..., sl], v), (k, name)
        for name in ("metrics", "counters", "flags"):
            assert torch.equal(getattr(pb, name)[:, sl], getattr(sb, name)), (k, name)
        for name in ("hand_metrics",):
            assert torch.equal(getattr(pb, name)[:, sl], getattr(sb, name)), (k, name)
        for name in ("state", "hand_state", "hand_step", "hand_success"):
            assert torch.equal(getattr(pb, name)[sl], getattr(sb, name)), (k, name)
        senv.close()
    assert not torch.equal(pb.metrics[0, :E], pb.metrics[0, E:2 * E])      # the replicas' weights differ, and so do their episodes
    penv.close()
    pop.close()


# ---------------------------------------------------------------------------------------------------------------- 3. against the shipped evaluator
@pytest.mark.parametrize("hidden,mode,confirm", [(64, "approach", 2), (128, "approach", 0), (128, "dock", None)])
def test_run_episodes_fused_equals_run_episodes(policies, suite, hidden, mode, confirm):
    pol = policies[hidden][1]
    cfg = _cfg(mode)
    ready = F.READY
    active = _active_mask(E).bool()
    out = []
    for fused in (True, False):
        env = ArmKinematicVecEnv(cfg, E, seed=3)
        env.set_obs_stride(64)
        if fused:
            out.append(ev.run_episodes_fused(env, pol._mlp, _opts(suite, mode), ready_cfg=ready, handoff_confirm_steps=confirm, active=active))
        else:
            out.append(ev.run_episodes(env, pol.predict, _opts(suite, mode), ready_cfg=ready, handoff_confirm_steps=confirm, active=active))
        env.close()
    (res, hand), (ref, ref_hand) = out
    F.assert_results_match(res, ref, "final")
    assert (hand is None) == (ref_hand is None) == (confirm is None)
    if hand is not None:
        F.assert_results_match(hand, ref_hand, "handoff")
    assert int(ref["step_count"].max()) >= 2


# ---------------------------------------------------------------------------------------------------------------- 4. / 5. evaluator on a population
def _bigtrain_cfg():
    return kcfg.to_env_config(kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"))


def _dock_cfg():
    d = kcfg.load_yaml_file(kcfg.builtin_config_dir() / "dock_workspace_handoff_noop_ft_12env.yaml")
    d["env"]["dock_reset"]["handoff_state_probability"] = 0.0
    return kcfg.to_env_config(d)


def _population(seeds, n_envs=16):
    from rl_brain_trainer_amd.population import ApproachPopulationPPO
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    env_cfg = _bigtrain_cfg()
    penv = ArmKinematicPopulationVecEnv(env_cfg, seeds, n_envs)
    pop = ApproachPopulationPPO(seeds, P.PPOConfig(n_steps=32, batch_size=128, n_epochs=2, hidden=64, learning_rate=3e-3), penv)
    return pop, penv, env_cfg


EVAL_KW = dict(episodes=4, seed=700001, stage_indices=[0, 3], handoff_confirm_steps=2, gate_config={"score_stage_index": 3})


@pytest.mark.parametrize("finisher", ["h64", "h256", None])
def test_population_evaluator_equals_per_replica_evaluations(tmp_path, finisher):
    """evaluate_workspace_expansion_population on a 3-replica ApproachPopulationPPO after one learn iteration against three
    evaluate_workspace_expansion(approach_policy=pop.replica(k).predict) calls: payloads equal (action-magnitude floats to the tolerance of
    the fused runner), the JSON files parse to the payloads.  Finisher: a 2x64 net (one-launch step), a 2x256 net (run_episodes), none."""
    pop, penv, env_cfg = _population([7, 8, 9])
    pop.learn(pop.n_envs * pop.cfg.n_steps)
    assert not torch.equal(pop.flat[0], pop.flat[1])
    fin = None if finisher is None else P.InferencePolicy(P.ActorCritic(int(finisher[1:]), DEV, seed=5).state_dict(), device=DEV)
    fcfg = None if finisher is None else _dock_cfg()
    roots = [tmp_path / f"r{k}" for k in range(3)]
    got = ev.evaluate_workspace_expansion_population(population=pop, finisher_policy=fin, approach_cfg=env_cfg, finisher_cfg=fcfg, artifact_roots=roots,
                                                     **EVAL_KW)
    assert len(got) == 3
    for k in range(3):
        ref = ev.evaluate_workspace_expansion(approach_policy=pop.replica(k).predict, finisher_policy=fin, approach_cfg=env_cfg, finisher_cfg=fcfg,
                                              artifact_root=tmp_path / f"ref{k}", obs_stride=pop.obs_w, **EVAL_KW)
        F.assert_payload_match(got[k], ref)
        assert json.loads((roots[k] / "workspace_eval_summary.json").read_text()) == json.loads(json.dumps(got[k]))
        assert json.loads((roots[k] / "stage_metrics.json").read_text()) == json.loads(json.dumps(got[k]["stage_metrics"]))
        assert json.loads((roots[k] / "best_model_selection_summary.json").read_text()) == json.loads(json.dumps(got[k]["best_model_selection"]))
    assert got[0]["target_rows"] != got[1]["target_rows"]
    pop.close()
    penv.close()


def test_population_evaluation_leaves_training_untouched():
    """parameters, Adam moments and env state after [iteration, evaluation, iteration] == after [iteration, iteration]: the evaluator
    disturbs neither the captured graphs, nor the training handle, nor the env"""
    out = []
    for evaluate in (True, False):
        pop, penv, env_cfg = _population([7, 8, 9])
        pop.learn(pop.n_envs * pop.cfg.n_steps)
        if evaluate:
            before = (pop.flat.clone(), pop.adam_m.clone(), pop.adam_v.clone(), {k: v.clone() for k, v in penv.info().items()}, penv.rng_state())
            ev.evaluate_workspace_expansion_population(population=pop, finisher_policy=None, approach_cfg=env_cfg, finisher_cfg=None, **EVAL_KW)
            after = (pop.flat, pop.adam_m, pop.adam_v, penv.info(), penv.rng_state())
            assert all(torch.equal(x, y) for x, y in zip(before[:3], after[:3]))
            assert all(torch.equal(before[3][k], after[3][k]) for k in before[3]) and np.array_equal(before[4], after[4])
        pop.learn(pop.n_envs * pop.cfg.n_steps)
        torch.cuda.synchronize()
        out.append((pop.flat.clone(), pop.adam_m.clone(), pop.adam_v.clone(), {k: v.clone() for k, v in penv.info().items()}, penv.rng_state(),
                    pop.obs_buf.clone()))
        pop.close()
        penv.close()
    a, b = out
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[5], b[5])
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3]) and np.array_equal(a[4], b[4])


# ---------------------------------------------------------------------------------------------------------------- 6. CLI
def test_train_cli_seeds_gate_equals_single_seed_runs(tmp_path):
    """train.py --seeds 7,8 with the gate on against --seed 7 and --seed 8 (the tiny config of tests/test_train_cli_gpu.py, 2x64 nets):
    per replica the same eval_history selection entries and final stage metrics (action floats to the tolerance), the same artefact files"""
    import yaml

    from rl_brain_trainer_amd import checkpoint, train

    cfg_dir = kcfg.builtin_config_dir()
    dock_dict = kcfg.load_yaml_file(cfg_dir / "dock_workspace_handoff_noop_ft_12env.yaml")
    dock_dict["env"]["dock_reset"]["handoff_state_probability"] = 0.0      # the reference's buffer file is not shipped
    dock_yaml = tmp_path / "dock.yaml"
    dock_yaml.write_text(yaml.safe_dump(dock_dict))
    fenv = ArmKinematicVecEnv(kcfg.to_env_config(dock_dict), 8, seed=1)
    fin = P.PPO(fenv, P.PPOConfig(n_steps=4, batch_size=32, n_epochs=1, hidden=64, seed=1), backend="hip", use_graphs=False)
    fin_zip = checkpoint.save(tmp_path / "finisher", fin)
    fenv.close()
    overlay = {"base_config": str(cfg_dir / "workspace_expansion_bigtrain.yaml"),
               "workspace_expansion": {"finisher_checkpoint": str(fin_zip), "finisher_config": str(dock_yaml), "eval_interval": 4096, "gate_eval_episodes": 3,
                                       "final_eval_episodes": 3, "init_approach_checkpoint": ""}}
    cfg_path = tmp_path / "run.yaml"
    cfg_path.write_text(yaml.safe_dump(overlay))
    common = ["--config", str(cfg_path), "--total-timesteps", "8192", "--n-envs", "256", "--n-steps", "16", "--batch-size", "1024", "--hidden", "64",
              "--log-every", "0"]
    pop_root = tmp_path / "pop"
    train.main(common + ["--run-id", "p", "--artifact-root", str(pop_root), "--seeds", "7,8"])
    files = ("eval_history.jsonl", "latest_checkpoint/model_latest.zip", "model_latest.zip", "training_summary.json", "config_resolved.yaml",
             "final_eval/stage_metrics.json", "final_eval/workspace_eval_summary.json", "final_eval/best_model_selection_summary.json", "stage_metrics.json",
             "gate_candidates/candidate_step_4096.zip", "gate_candidates/candidate_step_8192.zip", "gate_evals/eval_step_4096/workspace_eval_summary.json",
             "gate_evals/eval_step_8192/stage_metrics.json")
    for s in (7, 8):
        single = tmp_path / f"single_{s}"
        train.main(common + ["--run-id", f"s{s}", "--artifact-root", str(single), "--seed", str(s)])
        rep = pop_root / f"seed_{s}"
        for f in files:
            assert (single / f).exists() and (rep / f).exists(), (s, f)
        assert (single / "best_checkpoint/model_best_by_gate.zip").exists() == (rep / "best_checkpoint/model_best_by_gate.zip").exists()
        ha = [json.loads(l) for l in (rep / "eval_history.jsonl").read_text().splitlines()]
        hb = [json.loads(l) for l in (single / "eval_history.jsonl").read_text().splitlines()]
        assert [h["timesteps"] for h in ha] == [4096, 8192] == [h["timesteps"] for h in hb]
        for x, y in zip(ha, hb):
            x.pop("candidate"), y.pop("candidate")
            F.assert_payload_match(x, y, f"seed_{s}/history")
        ta, tb = (json.loads((r / "training_summary.json").read_text()) for r in (rep, single))
        F.assert_payload_match(ta["final_workspace_eval"]["stage_metrics"], tb["final_workspace_eval"]["stage_metrics"], f"seed_{s}/final")
    summ = json.loads((pop_root / "population_summary.json").read_text())
    assert [r["seed"] for r in summ["per_seed"]] == [7, 8]
