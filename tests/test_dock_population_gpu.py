"""Dock (Finisher) population on one env handle, on the GPU: tracker k of a DockReverseCurriculumPopulation, block k of a dock-mode
ArmKinematicPopulationVecEnv, replica k of DockPopulationPPO and seed s of `train_dock.py --seeds` are bit-identical to the single K = 1
objects with seed s_k -- while the replicas sit on different reverse-curriculum stages and share waves of the dock step kernel."""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden_config
from rl_brain_trainer_amd import finisher_tools as ft
from rl_brain_trainer_amd import native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEEDS = [7, 8, 9]
KP1_ERR_INVALID, KP1_ERR_UNSUPPORTED = -1, -4     # include/kp1.h
DOCK_CFG = "dock_workspace_handoff_noop_ft_12env_raw"     # 36-step episodes, handoff-state resets from the golden buffer


def _bytes(obj) -> bytes:
    return bytes(C.string_at(C.addressof(obj), C.sizeof(obj)))


def _stages(min_episodes: int) -> list[dict]:
    """a synthetic reverse curriculum that promotes on every `min_episodes` finished episodes (threshold 0) and overrides every value a stage
    can hold, the handoff filter included (so each stage has its own slice of the concatenated buffer)"""
    return [
        {"name": "close", "min_episodes": min_episodes, "window_episodes": 4, "success_rate_threshold": 0.0, "dock_residual_action_limit": 0.2,
         "close_bucket_probability": 1.0, "close_bucket_max_pos_error_m": 0.003, "handoff_state_probability": 0.3,
         "init_q_noise": [0.002] * 7},
        {"name": "mid", "min_episodes": min_episodes, "success_rate_threshold": 0.0, "action_delta_scale": 0.012, "close_bucket_probability": 0.5,
         "close_init_q_noise": [0.004, 0.006, 0.008, 0.006, 0.004, 0.004, 0.003], "close_bucket_max_ori_error_rad": 0.03,
         "close_bucket_min_pos_error_m": 0.001, "handoff_state_probability": 0.6, "handoff_state_max_action_l2": 0.3},
        {"name": "wide", "dock_delta_q_change_limit_scale": 0.5, "dock_residual_action_limit": 0.35, "close_bucket_probability": 0.1,
         "handoff_state_probability": 0.9, "handoff_state_max_action_l2": 0.5},
    ]


# ---------------------------------------------------------------------------------------------------------------- tracker
def test_dock_population_tracker_matches_reference_callback():
    """One population of three trackers, N = 5: golden trace 0 fed to replicas 0 and 2, trace 1 to replica 1, in ONE launch per step.  After
    every step each replica's stage and episode count are the reference callback's, each live record is resolved_stages(...)[stage] byte for
    byte; at the end each summary() is the trace's.  The golden table re-filters the handoff buffer per stage."""
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    g = json.loads((GOLDEN / "dock_reverse_curriculum.json").read_text())
    traces = [g["traces"][0], g["traces"][1], g["traces"][0]]
    n = len(traces[0]["steps"][0]["dones"])
    assert n == 5 and all(len(t["steps"]) == len(traces[0]["steps"]) for t in traces)
    cfg = load_golden_config(DOCK_CFG)
    env = ArmKinematicPopulationVecEnv(cfg, SEEDS, n, mode="dock")
    pcur = ft.DockReverseCurriculumPopulation(stages=g["stages"], window_episodes=g["window_episodes"], n_replicas=3, handoff_base_dirs=(GOLDEN,))
    pcur.attach(env)
    ref = ft.DockReverseCurriculum(stages=g["stages"], window_episodes=g["window_episodes"], handoff_base_dirs=(GOLDEN,))
    base = load_golden_config(DOCK_CFG)
    table = ref.resolved_stages(base, ref.stage_buffers(base))
    assert len({(t.handoff_offset, t.handoff_count) for t in table}) == len(table)   # every stage its own slice
    env.reset()
    for t in range(len(traces[0]["steps"])):
        bits = [[(2 if d else 0) | (4 if s else 0) for d, s in zip(tr["steps"][t]["dones"], tr["steps"][t]["success"])] for tr in traces]
        pcur.observe(torch.tensor(sum(bits, []), dtype=torch.uint8, device=DEV), n)
        live = pcur.live_records()
        for k, tr in enumerate(traces):
            st = pcur.read(k)
            assert (int(st.stage_index), int(st.stage_episode_count)) == (tr["steps"][t]["stage"], tr["steps"][t]["count"]), (t, k)
            assert _bytes(live[k]) == _bytes(table[int(st.stage_index)]), (t, k)
    stages = []
    for k, tr in enumerate(traces):
        assert json.loads(json.dumps(pcur.replica(k).summary())) == tr["summary"], k
        stages.append(pcur.replica(k).current_stage_index)
    assert stages[0] != stages[1], stages        # the replicas end on different stages
    pcur.close()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- env blocks
@pytest.mark.parametrize("comps", [False, True])
@pytest.mark.parametrize("n", [12, 96])
def test_dock_population_env_blocks_match_single_envs(n, comps):
    """K = 3 replicas of the dock env with a promoting reverse curriculum, against ArmKinematicVecEnv(seed=s_k) + its own
    DockReverseCurriculum.  Replicas 1 and 2 are reset (their rows only) at steps 11 and 23, so their episodes, and with them their
    promotions, run out of step with replica 0's.  Every step: observations, rewards, done bytes, terminal observations, every info plane
    (and the reward components); every 40 steps and at the end: PCG64 words and tracker bytes; after the run a full reset()."""
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    K, steps = len(SEEDS), 420
    stages = _stages(min_episodes=3 * n)
    cfg = load_golden_config(DOCK_CFG)
    assert cfg.c.dock_reset.handoff_state_probability > 0 and cfg.handoff_states
    pop = ArmKinematicPopulationVecEnv(cfg, SEEDS, n, reward_components=comps, mode="dock")
    pcur = ft.DockReverseCurriculumPopulation(stages=stages, window_episodes=4, n_replicas=K, handoff_base_dirs=(GOLDEN,))
    pcur.attach(pop)
    singles, curs = [], []
    for s in SEEDS:
        env = ArmKinematicVecEnv(load_golden_config(DOCK_CFG), n, seed=s, reward_components=comps)
        cur = ft.DockReverseCurriculum(stages=stages, window_episodes=4, handoff_base_dirs=(GOLDEN,))
        cur.attach(env)
        singles.append(env)
        curs.append(cur)
    assert np.array_equal(pop.rng_state(), np.concatenate([e.rng_state() for e in singles]))
    obs = pop.reset()
    for k, env in enumerate(singles):
        assert torch.equal(env.reset(), obs[pop.rows(k)]), k
    gen = torch.Generator(device=DEV).manual_seed(4321 + n)
    differ_at = None
    for t in range(steps):
        if t in (11, 23):
            k = 1 if t == 11 else 2
            mask = torch.zeros(K * n, dtype=torch.uint8, device=DEV)
            mask[pop.rows(k)] = 1
            pop.reset(mask=mask)
            singles[k].reset()
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
            for name, plane in env.info().items():
                assert torch.equal(plane, info[name][..., r]), (t, k, name)
            if comps:
                assert torch.equal(env.reward_components()[1], pop.reward_components()[1][:, r]), (t, k, "components")
        if t % 40 == 39 or t == steps - 1:
            assert np.array_equal(pop.rng_state(), np.concatenate([e.rng_state() for e in singles])), t
            now = [int(pcur.read(k).stage_index) for k in range(K)]
            for k, cur in enumerate(curs):
                assert _bytes(cur.read()) == _bytes(pcur.read(k)), (t, k)
            if differ_at is None and len(set(now)) > 1:
                differ_at = (t, now)
    assert differ_at is not None, "the replicas never sat on different stages"
    assert all(pcur.read(k).n_events >= 1 for k in range(K))
    # reset() after the promotions samples each block with its own replica's stage
    obs = pop.reset()
    info = pop.info()
    for k, env in enumerate(singles):
        assert torch.equal(env.reset(), obs[pop.rows(k)]), ("reset", k)
        for name, plane in env.info().items():
            assert torch.equal(plane, info[name][..., pop.rows(k)]), ("reset", k, name)
    assert np.array_equal(pop.rng_state(), np.concatenate([e.rng_state() for e in singles]))
    # each replica's config copy follows its own stage, as each single run's config does
    for k, cur in enumerate(curs):
        assert _bytes(pcur.replica(k).config.c) == _bytes(singles[k].config.c), k
        assert pcur.replica(k).config.handoff_states == singles[k].config.handoff_states
    with pytest.raises(ValueError, match="DockReverseCurriculumPopulation"):
        pop.apply_dock_training_stage({"dock_residual_action_limit": 0.1})
    pcur.close()
    pop.close()
    for cur, env in zip(curs, singles):
        cur.close()
        env.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_dock_population_refusals():
    """a bound handle refuses the fused policy + env step; the population tracker refuses an f64 handle, N % K != 0, a handle bound to an
    Approach population or carrying a single dock tracker; a bound handle refuses a single tracker and an Approach binding"""
    from rl_brain_trainer_amd import config as kcfg
    from rl_brain_trainer_amd.curriculum import PointCurriculumPopulation
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    g = json.loads((GOLDEN / "dock_reverse_curriculum.json").read_text())
    cfg = load_golden_config(DOCK_CFG)
    L = native.load()
    vp, i32 = C.c_void_p, C.c_int32
    L.kp1_dock_curriculum_create_population.argtypes = [vp, C.POINTER(ft._Stage), i32, i32, i32, C.POINTER(vp)]
    table = ft.DockReverseCurriculum(stages=g["stages"], window_episodes=8, handoff_base_dirs=(GOLDEN,)).resolved_stages(cfg)

    def create(env, k):
        out = C.c_void_p()
        return L.kp1_dock_curriculum_create_population(env._handle, table, len(table), 8, k, C.byref(out)), out

    # f64 handle, N % K, K > 16
    e64 = ArmKinematicVecEnv(cfg, 12, seed=1, real="f64")
    assert create(e64, 3)[0] == KP1_ERR_UNSUPPORTED
    e64.close()
    env = ArmKinematicVecEnv(cfg, 10, seed=1)
    assert create(env, 3)[0] == KP1_ERR_INVALID
    assert create(env, 17)[0] == KP1_ERR_INVALID
    # a handle carrying a single dock tracker
    single = ft.DockReverseCurriculum(stages=g["stages"], window_episodes=8, handoff_base_dirs=(GOLDEN,))
    single.attach(env)
    assert create(env, 2)[0] == KP1_ERR_UNSUPPORTED
    single.close()
    env.close()
    # a handle bound to an Approach population (an Approach-mode handle bound, then switched to dock)
    acfg = kcfg.to_env_config(kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"))
    aenv = ArmKinematicPopulationVecEnv(acfg, [1, 2], 8)
    acur = PointCurriculumPopulation(success_rate_threshold=0.5, window_episodes=4, min_episodes_per_stage=4, max_stage_index=acfg.n_stages - 1,
                                     initial_stage_indices=[0, 1])
    acur.attach(aenv)
    aenv.set_policy_mode("approach")
    L.kp1_set_mode(aenv._handle, 1)
    rc, _ = create(aenv, 2)
    assert rc != 0
    acur.close()
    aenv.close()
    # a bound dock population: no single tracker, no Approach binding, no fused step, step / reset in the dock mode only
    pop = ArmKinematicPopulationVecEnv(cfg, [1, 2], 6, mode="dock")
    pcur = ft.DockReverseCurriculumPopulation(stages=g["stages"], window_episodes=8, n_replicas=2, handoff_base_dirs=(GOLDEN,))
    pcur.attach(pop)
    with pytest.raises(native.Kp1Error, match="dock population"):
        ft.DockReverseCurriculum(stages=g["stages"], window_episodes=8, handoff_base_dirs=(GOLDEN,)).attach(pop)
    states = C.c_void_p()
    assert L.kp1_curriculum_create_population(0, 2, 0.5, 4, 4, 3, C.cast((C.c_int32 * 2)(0, 0), C.c_void_p), C.byref(states)) == 0
    assert L.kp1_bind_population_stages(pop._handle, states, 2) == KP1_ERR_UNSUPPORTED
    L.kp1_curriculum_destroy(0, states)
    from rl_brain_trainer_amd.mlp import MlpKernels

    mlp = MlpKernels(256, DEV, max_batch=64)
    pop.set_obs_stride(64)
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=DEV)   # noqa: E731
    with pytest.raises(native.Kp1Error, match="dock population"):
        mlp.forward_env_step(pop, z(12, 64), noise=z(12, 7), value=z(12), action=z(12, 7), log_prob=z(12), next_obs=z(12, 64), reward=z(12),
                             done=z(12, dt=torch.uint8), terminal_obs=z(12, 64))
    mlp.close()
    with pytest.raises(ValueError, match="mode"):
        pop.set_policy_mode("approach")
    L.kp1_set_mode(pop._handle, 0)
    with pytest.raises(native.Kp1Error, match="dock mode only"):
        pop.step(torch.zeros((12, 7), device=DEV))
    L.kp1_set_mode(pop._handle, 1)
    pop.step(torch.zeros((12, 7), device=DEV))
    # destroy unbinds: the handle steps in the ordinary dock form again and takes a single tracker
    pcur.close()
    pop.step(torch.zeros((12, 7), device=DEV))
    assert pop.dock_population is None
    pop.close()


# ---------------------------------------------------------------------------------------------------------------- trainer
BUFFERS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf", "term_obs_buf")


@pytest.mark.parametrize("use_graphs", [True, False])
def test_dock_population_ppo_matches_single_runs(use_graphs):
    """DockPopulationPPO (one env handle, one tracker launch per step) against K single PPO runs with their own DockReverseCurriculum, 4
    iterations: rollout buffers, parameters, Adam moments, adam_t, statistics and tracker bytes of replica k equal those of PPO(seed=s_k)"""
    from rl_brain_trainer_amd.population import DockPopulationPPO
    from rl_brain_trainer_amd.ppo import PPO, PPOConfig
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    N, K = 12, len(SEEDS)
    stages = _stages(min_episodes=N)
    pcfg = PPOConfig(n_steps=64, batch_size=128, n_epochs=2, hidden=64, learning_rate=3e-4, ent_coef=1e-3)
    penv = ArmKinematicPopulationVecEnv(load_golden_config(DOCK_CFG), SEEDS, N, mode="dock")
    pcur = ft.DockReverseCurriculumPopulation(stages=stages, window_episodes=4, n_replicas=K, handoff_base_dirs=(GOLDEN,))
    pop = DockPopulationPPO(SEEDS, dataclasses.replace(pcfg), penv, curriculum=pcur, use_graphs=use_graphs)
    singles = [PPO(ArmKinematicVecEnv(load_golden_config(DOCK_CFG), N, seed=s), dataclasses.replace(pcfg, seed=s),
                   curriculum=ft.DockReverseCurriculum(stages=stages, window_episodes=4, handoff_base_dirs=(GOLDEN,)), use_graphs=use_graphs)
               for s in SEEDS]
    for it in range(4):
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
            assert _bytes(p.curriculum.read()) == _bytes(pcur.read(k)), (it, k)
            assert p.curriculum.summary() == pop.replica(k).curriculum.summary(), (it, k)
            assert p.last_stats == pop.replica(k).last_stats, (it, k)
    assert all(pcur.summary(k)["history"] for k in range(K)), "a replica never promoted: the trackers were compared without a promotion"
    pop.close()
    pcur.close()
    penv.close()
    for p in singles:
        p.curriculum.close()
        p.env.close()


# ---------------------------------------------------------------------------------------------------------------- CLI
CLI_SEEDS = (3, 4, 5)


def _cli_yaml(tmp_path, stages) -> str:
    import yaml

    from rl_brain_trainer_amd import config as kcfg

    dock = kcfg.load_yaml_file(kcfg.builtin_config_dir() / "dock_workspace_handoff_noop_ft_12env.yaml")
    shutil.copy(GOLDEN / "handoff_state_buffer.json", tmp_path / "handoff_state_buffer.json")
    dock["env"]["dock_reset"]["handoff_state_buffer_path"] = "handoff_state_buffer.json"
    dock["env"]["dock_reset"]["handoff_state_probability"] = 0.5
    dock.setdefault("training", {})["dock_reverse_curriculum"] = {"enabled": True, "window_episodes": 4, "stages": stages}
    path = tmp_path / "dock.yaml"
    path.write_text(yaml.safe_dump(dock))
    return str(path)


# Seeds end on different stages under this table.  A stage waits for min_episodes finished episodes whose newest 4 reach its threshold, and
# the successes of the barely trained policies differ from seed to seed: over 3072 steps per seed, seed 3 leaves "wide" an episode round
# (36 env steps) later than seeds 4 and 5, and then has too few episodes left to reach "hold"'s min_episodes ("hold" overrides nothing).
CLI_STAGES = [
    {"name": "close", "min_episodes": 12, "window_episodes": 4, "success_rate_threshold": 0.25, "close_bucket_probability": 1.0,
     "close_bucket_max_pos_error_m": 0.002, "handoff_state_probability": 0.0, "dock_residual_action_limit": 0.1},
    {"name": "mid", "min_episodes": 12, "window_episodes": 4, "success_rate_threshold": 0.5, "close_bucket_probability": 0.5,
     "handoff_state_probability": 0.5, "handoff_state_max_action_l2": 0.3},
    {"name": "wide", "min_episodes": 12, "window_episodes": 4, "success_rate_threshold": 0.75, "close_bucket_probability": 0.1,
     "handoff_state_probability": 0.9, "dock_residual_action_limit": 0.35},
    {"name": "hold", "min_episodes": 40, "window_episodes": 4, "success_rate_threshold": 0.5},
    {"name": "final", "dock_delta_q_change_limit_scale": 0.5},
]


def _artefacts(root):
    from rl_brain_trainer_amd import checkpoint

    z = root / "model_latest.zip"
    summ = json.loads((root / "training_summary.json").read_text())
    return {"policy": checkpoint.load_policy_state_dict(z), "optimizer": checkpoint.load_optimizer_state_dict(z), "data": checkpoint.load_data(z),
            "eval": json.loads((root / "dock_eval" / "dock_eval_summary.json").read_text()), "curriculum": summ["dock_reverse_curriculum"],
            "num_timesteps": summ["num_timesteps"], "dock_eval_summary": summ["dock_eval_summary"]}


def _assert_same(a, b, what):
    assert a["policy"].keys() == b["policy"].keys() and all(torch.equal(a["policy"][k], b["policy"][k]) for k in a["policy"]), what
    for i, st in b["optimizer"]["state"].items():
        for name, v in st.items():
            assert torch.equal(a["optimizer"]["state"][i][name], v), (what, i, name)
    for key in ("eval", "curriculum", "num_timesteps", "dock_eval_summary"):
        assert a[key] == b[key], (what, key)
    for key in ("num_timesteps", "_n_updates", "gamma", "n_epochs"):
        assert a["data"].get(key) == b["data"].get(key), (what, key)


@pytest.mark.parametrize("log_every", [0, 1])
def test_train_dock_cli_seeds_matches_seed_runs(tmp_path, log_every):
    """train_dock --seeds 3,4,5 on one handle: every seed's model, optimiser state, dock evaluation and reverse-curriculum block equal those of
    --seed s, and the seeds end on different stages (each is evaluated on its own stage's config)"""
    from rl_brain_trainer_amd import train_dock

    cfg_path = _cli_yaml(tmp_path, CLI_STAGES)
    common = ["--config", cfg_path, "--total-timesteps", "3072", "--n-envs", "12", "--n-steps", "64", "--batch-size", "256", "--hidden", "64",
              "--eval-episodes", "24", "--log-every", str(log_every)]
    root = tmp_path / "pop"
    train_dock.main(common + ["--run-id", "p", "--artifact-root", str(root), "--seeds", ",".join(map(str, CLI_SEEDS))])
    finals = []
    for s in CLI_SEEDS:
        single = tmp_path / f"single_{s}"
        train_dock.main(common + ["--run-id", f"s{s}", "--artifact-root", str(single), "--seed", str(s)])
        a, b = _artefacts(root / f"seed_{s}"), _artefacts(single)
        _assert_same(a, b, s)
        finals.append(a["curriculum"]["stage_index"])
    assert len(set(finals)) > 1, finals


def test_train_dock_cli_seeds_resume(tmp_path):
    """the two-phase Finisher recipe as a population: phase 1 from scratch, phase 2 --resume-from the phase-1 root equals each seed's own
    two-phase run; and --resume-from <zip> equals --seed s --resume-from <zip>"""
    from rl_brain_trainer_amd import train_dock

    cfg_path = _cli_yaml(tmp_path, CLI_STAGES)
    common = ["--config", cfg_path, "--total-timesteps", "1536", "--n-envs", "12", "--n-steps", "64", "--batch-size", "256", "--hidden", "64",
              "--eval-episodes", "12", "--log-every", "0"]
    seeds = ",".join(map(str, CLI_SEEDS))
    p1, p2 = tmp_path / "pop1", tmp_path / "pop2"
    train_dock.main(common + ["--run-id", "p1", "--artifact-root", str(p1), "--seeds", seeds])
    train_dock.main(common + ["--run-id", "p2", "--artifact-root", str(p2), "--seeds", seeds, "--resume-from", str(p1)])
    for s in CLI_SEEDS:
        s1, s2 = tmp_path / f"s1_{s}", tmp_path / f"s2_{s}"
        train_dock.main(common + ["--run-id", "s1", "--artifact-root", str(s1), "--seed", str(s)])
        train_dock.main(common + ["--run-id", "s2", "--artifact-root", str(s2), "--seed", str(s), "--resume-from", str(s1 / "model_latest.zip")])
        _assert_same(_artefacts(p2 / f"seed_{s}"), _artefacts(s2), ("two-phase", s))
        assert _artefacts(p2 / f"seed_{s}")["num_timesteps"] == 2 * _artefacts(p1 / f"seed_{s}")["num_timesteps"]
    # one zip for every seed
    zip_path = str(tmp_path / "s1_3" / "model_latest.zip")
    p3 = tmp_path / "pop3"
    train_dock.main(common + ["--run-id", "p3", "--artifact-root", str(p3), "--seeds", "4,5", "--resume-from", zip_path])
    for s in (4, 5):
        single = tmp_path / f"z_{s}"
        train_dock.main(common + ["--run-id", "z", "--artifact-root", str(single), "--seed", str(s), "--resume-from", zip_path])
        _assert_same(_artefacts(p3 / f"seed_{s}"), _artefacts(single), ("zip", s))
