"""Approach population on one env handle, on the GPU: block k of an ArmKinematicPopulationVecEnv with a PointCurriculumPopulation, tracker k
of that population, replica k of ApproachPopulationPPO and seed s of `train.py --seeds` are bit-identical to the single K = 1 objects with
seed s_k -- while the replicas sit on different curriculum stages and share waves of the step kernel."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from rl_brain_trainer_amd import config as kcfg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEEDS = [7, 8, 9]
INITIAL_STAGES = [0, 2, 5]


def _env_cfg():
    cfg = kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml")
    env_cfg = kcfg.to_env_config(cfg)
    assert env_cfg.c.curriculum_enabled and env_cfg.n_stages >= 8
    return env_cfg


def _tracker_bytes(st) -> bytes:
    return bytes(C.string_at(C.addressof(st), C.sizeof(st)))


def _tracker_kwargs(env_cfg, window: int, min_episodes: int, threshold: float = 0.0) -> dict:
    return {"success_rate_threshold": threshold, "window_episodes": window, "min_episodes_per_stage": min_episodes,
            "max_stage_index": env_cfg.n_stages - 1}


# ---------------------------------------------------------------------------------------------------------------- env + tracker
@pytest.mark.parametrize("n", [16, 96])
def test_population_env_blocks_match_single_envs(n):
    """K = 3 replicas on stages [0, 2, 5] with a promoting tracker (threshold 0: a promotion per `n` finished episodes).  N = 16 puts four
    replicas' envs in one 64-lane wave, N = 96 a replica boundary inside a wave.  Every step: observations, rewards, done bytes, terminal
    observations and every info plane of block k equal those of ArmKinematicVecEnv(seed=s_k) + its own PointCurriculum; every 50 steps and
    at the end: the PCG64 words and the tracker bytes."""
    from rl_brain_trainer_amd.curriculum import PointCurriculum, PointCurriculumPopulation
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    env_cfg = _env_cfg()
    K, steps = len(SEEDS), 420
    kw = _tracker_kwargs(env_cfg, window=16, min_episodes=n)
    pop = ArmKinematicPopulationVecEnv(env_cfg, SEEDS, n)
    pcur = PointCurriculumPopulation(**kw, initial_stage_indices=INITIAL_STAGES)
    pcur.attach(pop)
    singles = [ArmKinematicVecEnv(env_cfg, n, seed=s) for s in SEEDS]
    curs = [PointCurriculum(**kw, initial_stage_index=st) for st in INITIAL_STAGES]
    for env, cur in zip(singles, curs):
        cur.attach(env)
    assert np.array_equal(pop.rng_state(), np.concatenate([e.rng_state() for e in singles]))
    obs = pop.reset()
    for k, env in enumerate(singles):
        assert torch.equal(env.reset(), obs[pop.rows(k)]), k
    gen = torch.Generator(device=DEV).manual_seed(1234 + n)
    stages_seen: list[set[int]] = [set() for _ in range(K)]
    for t in range(steps):
        act = torch.rand((K * n, 7), generator=gen, device=DEV) * 2.4 - 1.2
        pop.step(act)
        pcur.observe(pop.done, n)
        for k, (env, cur) in enumerate(zip(singles, curs)):
            env.step(act[pop.rows(k)].contiguous())
            cur.observe(env.done, n)
        info = pop.info()
        for k, env in enumerate(singles):
            r = pop.rows(k)
            assert torch.equal(env.obs, pop.obs[r]), (t, k, "obs")
            assert torch.equal(env.reward, pop.reward[r]), (t, k, "reward")
            assert torch.equal(env.done, pop.done[r]), (t, k, "done")
            assert torch.equal(env.terminal_obs, pop.terminal_obs[r]), (t, k, "terminal_obs")
            one = env.info()
            for name, plane in one.items():
                assert torch.equal(plane, info[name][..., r]), (t, k, name)
            stages_seen[k].update(int(v) for v in info["stage_index"][r].unique().tolist())
        if t % 50 == 49 or t == steps - 1:
            assert np.array_equal(pop.rng_state(), np.concatenate([e.rng_state() for e in singles])), t
            for k, cur in enumerate(curs):
                assert _tracker_bytes(cur.read()) == _tracker_bytes(pcur.read(k)), (t, k)
                assert cur.summary() == pcur.summary(k) == pcur.replica(k).summary(), (t, k)
    finals = [pcur.read(k) for k in range(K)]
    assert all(st.n_events >= 2 for st in finals), [st.n_events for st in finals]   # every replica promoted, at its own steps
    assert len({st.stage_index for st in finals}) == K, [st.stage_index for st in finals]
    # the auto-resets drew from each replica's own stages (stage_index plane: the stage of the env's last reset)
    assert all(max(stages_seen[k]) > INITIAL_STAGES[k] for k in range(K)), stages_seen
    assert stages_seen[0] != stages_seen[2], stages_seen
    pcur.close()
    pop.close()
    for cur, env in zip(curs, singles):
        cur.close()
        env.close()


@pytest.mark.parametrize("n", [16, 96, 5000])
def test_population_tracker_matches_single_trackers(n):
    """synthetic done streams: replica k finishes episodes at its own rate (the same episodes per step at every N) and succeeds with its own
    probability (threshold 0.5, so the replicas promote at different steps); one step in three ends nothing (the early-out).  N = 5000 covers
    more than one 4096-env block, and its step 120 -- every env ends -- the tracker's whole-wave path."""
    from rl_brain_trainer_amd.curriculum import PointCurriculum, PointCurriculumPopulation

    K, steps = 4, 160
    kw = {"success_rate_threshold": 0.5, "window_episodes": 32, "min_episodes_per_stage": 48, "max_stage_index": 9}
    init = [0, 3, 1, 9]
    pcur = PointCurriculumPopulation(**kw, initial_stage_indices=init)
    curs = [PointCurriculum(**kw, initial_stage_index=s) for s in init]
    g = np.random.default_rng(n)
    end_p = np.array([0.05, 0.2, 0.1, 0.3]) * 16 / n
    succ_p = np.array([0.9, 0.6, 0.3, 0.8])
    for t in range(steps):
        d = np.zeros((K, n), dtype=np.uint8)
        if t % 3 != 2:
            p_end = np.ones(K) if (n == 5000 and t == 120) else end_p
            ended = g.random((K, n)) < p_end[:, None]
            trunc = g.random((K, n)) < 0.5
            success = g.random((K, n)) < succ_p[:, None]
            d = np.where(ended, np.where(trunc, 2, 1) | np.where(success, 4, 0), 0).astype(np.uint8)
        dones = torch.from_numpy(d.reshape(-1)).to(DEV)
        pcur.observe(dones, n)
        for k, cur in enumerate(curs):
            cur.observe(dones[k * n:(k + 1) * n].contiguous(), n)
        if t % 10 == 9:
            for k, cur in enumerate(curs):
                assert _tracker_bytes(cur.read()) == _tracker_bytes(pcur.read(k)), (t, k)
    events = [[(e["from_stage_index"], e["total_timesteps"]) for e in pcur.summary(k)["history"]] for k in range(K)]
    assert sum(1 for ev in events if ev) >= 2, events
    first = [ev[0][1] for ev in events if ev]
    assert len(set(first)) > 1, events      # replicas promoted at different steps
    assert not events[3]                    # the one at max_stage_index never promotes
    pcur.close()
    for cur in curs:
        cur.close()


# ---------------------------------------------------------------------------------------------------------------- trainer
BUFFERS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf", "term_obs_buf")


@pytest.mark.parametrize("use_graphs", [True, False])
def test_approach_population_ppo_matches_single_runs(use_graphs):
    """ApproachPopulationPPO (one env handle, one tracker launch per step) against K single PPO runs, 3 iterations: rollout buffers,
    parameters, Adam moments, statistics and tracker bytes of replica k equal those of PPO(seed=s_k)"""
    from rl_brain_trainer_amd.curriculum import PointCurriculum, PointCurriculumPopulation
    from rl_brain_trainer_amd.population import ApproachPopulationPPO
    from rl_brain_trainer_amd.ppo import PPO, PPOConfig
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    env_cfg = _env_cfg()
    N, K = 16, len(SEEDS)
    kw = _tracker_kwargs(env_cfg, window=4, min_episodes=4)
    pcfg = PPOConfig(n_steps=64, batch_size=256, n_epochs=3, hidden=64, learning_rate=3e-4, ent_coef=1e-3)
    penv = ArmKinematicPopulationVecEnv(env_cfg, SEEDS, N)
    pcur = PointCurriculumPopulation(**kw, initial_stage_indices=INITIAL_STAGES)
    pop = ApproachPopulationPPO(SEEDS, dataclasses.replace(pcfg), penv, curriculum=pcur, use_graphs=use_graphs)
    singles = [PPO(ArmKinematicVecEnv(env_cfg, N, seed=s), dataclasses.replace(pcfg, seed=s), curriculum=PointCurriculum(**kw, initial_stage_index=st),
                   use_graphs=use_graphs) for s, st in zip(SEEDS, INITIAL_STAGES)]
    stages_differ = False
    for it in range(3):
        pop.collect_rollouts()
        for p in singles:
            p.collect_rollouts()
        torch.cuda.synchronize()
        for k, p in enumerate(singles):
            sl = slice(k * N, (k + 1) * N)
            for name in BUFFERS:
                assert torch.equal(getattr(p, name), getattr(pop, name)[:, sl]), (it, name, k)
        pop.train()
        for p in singles:
            p.train()
        torch.cuda.synchronize()
        for k, p in enumerate(singles):
            assert torch.equal(p.policy.flat, pop.flat[k]), (it, k)
            assert torch.equal(p.adam_m, pop.adam_m[k]) and torch.equal(p.adam_v, pop.adam_v[k]), (it, k)
            assert p.adam_t == pop.adam_t and p.num_timesteps == pop.num_timesteps, (it, k)
            assert _tracker_bytes(p.curriculum.read()) == _tracker_bytes(pcur.read(k)), (it, k)
            assert p.curriculum.summary() == pop.replica(k).curriculum.summary(), (it, k)
            assert p.last_stats == pop.replica(k).last_stats, (it, k)
        stages = [pcur.read(k).stage_index for k in range(K)]
        stages_differ |= len(set(stages)) > 1
    assert stages_differ, "the replicas never sat on different stages"
    assert any(pcur.summary(k)["history"] for k in range(K)), "no replica promoted: the trackers were compared without a promotion"
    pop.close()
    pcur.close()
    penv.close()
    for p in singles:
        p.curriculum.close()
        p.env.close()


def test_approach_population_ppo_recaptures_after_a_stage_binding():
    """binding the population tracker bumps launch_args_version of every replica view, so a captured rollout is captured again"""
    from rl_brain_trainer_amd.curriculum import PointCurriculumPopulation
    from rl_brain_trainer_amd.population import ApproachPopulationPPO
    from rl_brain_trainer_amd.ppo import PPOConfig
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    env_cfg = _env_cfg()
    penv = ArmKinematicPopulationVecEnv(env_cfg, [7, 8], 16)
    pop = ApproachPopulationPPO([7, 8], PPOConfig(n_steps=16, batch_size=64, n_epochs=1, hidden=64), penv)
    pop.collect_rollouts()
    graph = pop._rollout_graph
    assert graph is not None
    pcur = PointCurriculumPopulation(**_tracker_kwargs(env_cfg, 4, 4), initial_stage_indices=[0, 3])
    before = pop.envs[0].launch_args_version
    pcur.attach(penv)
    assert pop.envs[0].launch_args_version == pop.envs[1].launch_args_version == before + 1
    pop.collect_rollouts()
    assert pop._rollout_graph is not graph
    pop.close()
    pcur.close()
    penv.close()


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_train_cli_seeds_runs_on_one_env_handle(tmp_path, monkeypatch):
    """train.py --seeds 7,8 builds ONE ArmKinematicPopulationVecEnv of 2 x 16 envs (no per-seed handle), and seed s's model_latest.zip
    holds the policy and optimiser state of train.py --seed s"""
    import yaml

    from rl_brain_trainer_amd import checkpoint, train, vec_env

    made = []
    real_init = vec_env.ArmKinematicVecEnv.__init__

    def spy(self, *a, **k):
        made.append((type(self).__name__, a[1] if len(a) > 1 else k.get("n_envs")))
        real_init(self, *a, **k)

    monkeypatch.setattr(vec_env.ArmKinematicVecEnv, "__init__", spy)
    overlay = {"base_config": str(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"),
               "workspace_expansion": {"init_approach_checkpoint": "", "finisher_checkpoint": ""}}
    cfg_path = tmp_path / "run.yaml"
    cfg_path.write_text(yaml.safe_dump(overlay))
    common = ["--config", str(cfg_path), "--total-timesteps", "2048", "--n-envs", "16", "--n-steps", "64", "--batch-size", "256", "--hidden", "64",
              "--log-every", "0"]
    pop_root = tmp_path / "pop"
    train.main(common + ["--run-id", "p", "--artifact-root", str(pop_root), "--seeds", "7,8"])
    assert made == [("ArmKinematicPopulationVecEnv", 32)], made
    for s in (7, 8):
        single_root = tmp_path / f"single_{s}"
        train.main(common + ["--run-id", f"s{s}", "--artifact-root", str(single_root), "--seed", str(s)])
        a_zip, b_zip = pop_root / f"seed_{s}" / "model_latest.zip", single_root / "model_latest.zip"
        a, b = checkpoint.load_policy_state_dict(a_zip), checkpoint.load_policy_state_dict(b_zip)
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), s
        oa, ob = checkpoint.load_optimizer_state_dict(a_zip), checkpoint.load_optimizer_state_dict(b_zip)
        for i, st in ob["state"].items():
            for name, v in st.items():
                assert torch.equal(oa["state"][i][name], v), (s, i, name)
