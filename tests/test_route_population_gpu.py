"""Route-curriculum population on the GPU: replica k of a population -- MLP handle at 80-float observations, block k of a RoutePopulationVecEnv,
tracker k of a RoutePrefixCurriculumPopulation, replica k of RoutePopulationPPO and seed s of `train_route --seeds` -- is bit-identical to the
single K = 1 object with seed s_k."""
from __future__ import annotations

import ctypes as C
import dataclasses
import json

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import route_config as rcfg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _cfg(sequence: bool = True, route_keys: bool = True) -> dict:
    cfgd = json.loads((GOLDEN / "configs" / "route_curriculum_prefix120_routeobs_sequence2.json").read_text())
    cfgd["route"].setdefault("sequence", {})["enabled"] = sequence
    cfgd["route"].setdefault("observation", {})["include_route_keys"] = route_keys
    return cfgd


# ---------------------------------------------------------------------------------------------------------------- MLP at 80 floats
@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("n", [256, 200, 33, 1])
@pytest.mark.parametrize("normalize_mode", [1, 2])
def test_population_mlp_route_observation_matches_single_handles(hidden, n, normalize_mode):
    from rl_brain_trainer_amd import mlp
    from rl_brain_trainer_amd.ppo import ActorCritic

    K, total, IN, W = 3, 1024, 80, 128
    g = torch.Generator(device="cpu").manual_seed(hidden + n + 80)
    pols = [ActorCritic(hidden, DEV, seed=11 + k, obs_dim=IN) for k in range(K)]
    for p in pols:
        p.flat.add_(0.05 * torch.randn(p.numel, generator=g).to(DEV))
    P = pols[0].numel
    pop = mlp.MlpKernels(hidden, DEV, max_batch=n, obs_dim=IN, replicas=K)
    singles = [mlp.MlpKernels(hidden, DEV, max_batch=n, obs_dim=IN) for _ in range(K)]
    flat = torch.stack([p.flat for p in pols]).contiguous()
    pop.pack(flat)
    for s, p in zip(singles, pols):
        s.pack(p.flat)

    obs = torch.zeros((K * n, W), device=DEV)
    obs[:, :IN] = torch.randn((K * n, IN), generator=g).to(DEV)
    noise = torch.randn((K * n, 7), generator=g).to(DEV)
    outs = {k: torch.empty(shape, device=DEV) for k, shape in (("mean", (K * n, 7)), ("value", (K * n,)), ("action", (K * n, 7)),
                                                                  ("clipped", (K * n, 7)), ("log_prob", (K * n,)))}
    pop.forward(obs, noise=noise, **outs)
    for k, s in enumerate(singles):
        r = slice(k * n, (k + 1) * n)
        one = {name: torch.empty_like(t[r]) for name, t in outs.items()}
        s.forward(obs[r].contiguous(), noise=noise[r].contiguous(), **one)
        for name in one:
            assert torch.equal(one[name], outs[name][r]), (name, k)

    sobs = torch.zeros((total, W), device=DEV)
    sobs[:, :IN] = torch.randn((total, IN), generator=g).to(DEV)
    act = torch.randn((total, 7), generator=g).to(DEV)
    old_logp = (-8.0 + torch.randn(total, generator=g)).to(DEV)
    adv = torch.randn(total, generator=g).to(DEV)
    ret = torch.randn(total, generator=g).to(DEV)
    idx = torch.stack([torch.randperm(total, generator=g)[:n] for _ in range(K)]).to(DEV).contiguous()
    adv_stats = None
    if normalize_mode == 2:
        a = adv[idx]
        std = a.std(1) if n > 1 else torch.zeros(K, device=a.device)     # one row: the kernels' own definition, 1 / (0 + 1e-8)
        adv_stats = torch.stack([a.mean(1), 1.0 / (std + 1e-8)], dim=1).float().contiguous()
    kw = dict(clip_range=0.2, ent_coef=1e-3, vf_coef=0.5, inv_count=1.0 / n)
    grad = torch.zeros((K, P), device=DEV)
    stats = torch.zeros((K, 4), device=DEV)
    m, v = torch.zeros_like(grad), torch.zeros_like(grad)
    params = flat.clone()
    pop.set_step_count(0)
    for _ in range(2):
        pop.loss_grad(sobs, idx, n, act, old_logp, adv, ret, grad_out=grad, stats_out=stats, adv_stats=adv_stats, **kw)
        pop.adam_step(params, grad, m, v, lr=3e-4, eps=1e-5, max_grad_norm=0.5, step=0, fused_norm=True)
    for k, s in enumerate(singles):
        gk, sk = torch.zeros(P, device=DEV), torch.zeros(4, device=DEV)
        pk, mk, vk = flat[k].clone(), torch.zeros(P, device=DEV), torch.zeros(P, device=DEV)
        s.set_step_count(0)
        for _ in range(2):
            s.loss_grad(sobs, idx[k].contiguous(), n, act, old_logp, adv, ret, grad_out=gk, stats_out=sk,
                        adv_stats=None if adv_stats is None else adv_stats[k].contiguous(), **kw)
            s.adam_step(pk, gk, mk, vk, lr=3e-4, eps=1e-5, max_grad_norm=0.5, step=0, fused_norm=True)
        torch.cuda.synchronize()
        for name, a_, b_ in (("grad", gk, grad[k]), ("stats", sk, stats[k]), ("params", pk, params[k]), ("m", mk, m[k]), ("v", vk, v[k])):
            assert torch.equal(a_, b_), (name, k)
    assert not torch.equal(params[0], params[1])
    pop.close()
    for s in singles:
        s.close()


# ---------------------------------------------------------------------------------------------------------------- env and tracker
SEEDS, N = [11, 12, 40], 16


def _envs(cfgd, max_route_index=40):
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv, RouteVecEnv

    route_q = rcfg.load_route_q(GOLDEN / "synthetic_route.json")
    base = kcfg.to_env_config(cfgd)
    pop = RoutePopulationVecEnv(base, rcfg.route_config_from_dict(cfgd, max_route_index=max_route_index), route_q, SEEDS, N)
    singles = [RouteVecEnv(base, rcfg.route_config_from_dict(cfgd, max_route_index=max_route_index), route_q, N, seed=s) for s in SEEDS]
    return pop, singles


def _compare_step(pop, singles, what):
    pi = pop.info()
    for k, e in enumerate(singles):
        r = pop.rows(k)
        for name, a, b in (("obs", e.obs, pop.obs[r]), ("reward", e.reward, pop.reward[r]), ("done", e.done, pop.done[r]),
                           ("terminal_obs", e.terminal_obs, pop.terminal_obs[r])):
            assert torch.equal(a, b), (what, name, k)
        for key, t in e.info().items():
            u = pi[key]
            if u.dim() >= 1 and u.shape[-1] == pop.n_envs:
                u = u[..., r]
            assert torch.equal(t.cpu(), u.cpu()), (what, key, k)


@pytest.mark.parametrize("sequence", [True, False])
@pytest.mark.parametrize("route_keys", [True, False])
def test_population_env_blocks_match_single_envs(sequence, route_keys):
    pop, singles = _envs(_cfg(sequence, route_keys))
    assert pop.obs_dim == (80 if route_keys else 56) and pop.n_envs == len(SEEDS) * N
    # every replica its own window: the resets of block k must read window k
    for k, (lo, hi) in enumerate([(1, 10), (5, 40), (1, 120)]):
        pop.set_replica_window(k, min_route_index=lo, max_route_index=hi)
        singles[k].set_route_window(min_route_index=lo, max_route_index=hi)
    pop.reset()
    for e in singles:
        e.reset()
    _compare_step(pop, singles, "reset")
    g = torch.Generator(device="cpu").manual_seed(5)
    ended = 0
    for t in range(200):
        a = (0.6 * torch.randn((len(SEEDS) * N, 7), generator=g)).clamp(-1, 1).to(DEV)
        pop.step(a)
        for k, e in enumerate(singles):
            e.step(a[pop.rows(k)].contiguous())
        _compare_step(pop, singles, t)
        ended += int((pop.done & 3).ne(0).sum())
    assert ended > 0, "no episode ended: the auto-reset path was not compared"
    for k, e in enumerate(singles):
        assert np.array_equal(e.rng_state(), pop.rng_state()[k * N:(k + 1) * N]), k
    pop.close()
    for e in singles:
        e.close()


def _tracker_bytes(st) -> bytes:
    return bytes(C.string_at(C.addressof(st), C.sizeof(st)))


def test_population_tracker_matches_single_trackers():
    from rl_brain_trainer_amd.route_curriculum import RoutePrefixCurriculumDevice, RoutePrefixCurriculumPopulation, build_prefix_stages

    cfgd = _cfg()
    pop, singles = _envs(cfgd, max_route_index=120)
    kw = dict(stages=build_prefix_stages([10, 20, 30, 40]), promotion_success_rate=0.0, promotion_route_ready_hit_rate=0.0,
              promotion_orientation_hit_rate=0.0, promotion_max_regression_rate=1.0, window_episodes=12, min_episodes_per_stage=12)
    pcur = RoutePrefixCurriculumPopulation(**kw)
    pcur.attach(pop)
    scur = [RoutePrefixCurriculumDevice(**kw) for _ in SEEDS]
    for c, e in zip(scur, singles):
        c.attach(e)
    pop.reset()
    for e in singles:
        e.reset()
    g = torch.Generator(device="cpu").manual_seed(9)
    stages_seen = set()
    for t in range(260):
        # staggered masked resets (replica k restarts half its envs at step 10 + 15 k): the replicas' episodes end, and so promote, at
        # different steps
        for k in range(len(SEEDS)):
            if t == 10 + 15 * k:
                mask = torch.zeros(pop.n_envs, dtype=torch.uint8, device=DEV)
                mask[k * N:k * N + N // 2] = 1
                pop.reset(mask=mask)
                singles[k].reset(mask=mask[pop.rows(k)].clone())
        a = (0.6 * torch.randn((len(SEEDS) * N, 7), generator=g)).clamp(-1, 1).to(DEV)
        pop.step(a)
        for k, e in enumerate(singles):
            e.step(a[pop.rows(k)].contiguous())
        pcur.observe(pop.done, N)
        for c, e in zip(scur, singles):
            c.observe(e.done, N)
        stages = []
        for k, (c, e) in enumerate(zip(scur, singles)):
            s_one, s_pop = c.read(), pcur.read(k)
            assert _tracker_bytes(s_one) == _tracker_bytes(s_pop), (t, k)
            assert pop.window(k) == (e.route_cfg.reset.min_route_index, e.route_cfg.reset.max_route_index), (t, k)
            assert pcur.summary(k) == c.summary(), (t, k)
            stages.append(int(s_pop.stage_index))
        stages_seen.add(tuple(stages))
        assert torch.equal(pop.obs[:, :pop.obs_dim], torch.cat([e.obs for e in singles])), t
    assert any(len(set(s)) > 1 for s in stages_seen), f"the replicas always promoted together: {sorted(stages_seen)}"
    assert max(max(s) for s in stages_seen) > 0
    pcur.close()
    for c in scur:
        c.close()
    pop.close()
    for e in singles:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- trainer
BUFFERS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf")


def _curriculum_kwargs():
    from rl_brain_trainer_amd.route_curriculum import build_prefix_stages

    return dict(stages=build_prefix_stages([10, 20, 30]), promotion_success_rate=0.0, promotion_route_ready_hit_rate=0.0,
                promotion_orientation_hit_rate=0.0, promotion_max_regression_rate=1.0, window_episodes=16, min_episodes_per_stage=16)


@pytest.fixture(scope="module")
def init_checkpoint(tmp_path_factory):
    """a 2x64 route policy after one PPO iteration, saved as train_route saves model_latest"""
    from rl_brain_trainer_amd import checkpoint
    from rl_brain_trainer_amd.ppo import PPO, PPOConfig
    from rl_brain_trainer_amd.route_env import RouteVecEnv

    cfgd = _cfg()
    env_cfg = kcfg.to_env_config(cfgd)
    env = RouteVecEnv(env_cfg, rcfg.route_config_from_dict(cfgd, max_route_index=10), rcfg.load_route_q(GOLDEN / "synthetic_route.json"), 16, seed=3)
    ppo = PPO(env, PPOConfig(n_steps=64, batch_size=256, n_epochs=2, hidden=64, learning_rate=3e-4, seed=3), use_graphs=False)
    ppo.collect_rollouts()
    ppo.train()
    path = tmp_path_factory.mktemp("init") / "model_latest"
    checkpoint.save(path, ppo, env_cfg)
    env.close()
    return str(path) + ".zip"


@pytest.mark.parametrize("use_graphs", [True, False])
def test_route_population_ppo_matches_single_runs(init_checkpoint, use_graphs):
    from rl_brain_trainer_amd.population import RoutePopulationPPO
    from rl_brain_trainer_amd.ppo import PPO, PPOConfig
    from rl_brain_trainer_amd.route_curriculum import RoutePrefixCurriculumDevice, RoutePrefixCurriculumPopulation
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv, RouteVecEnv

    seeds, n_envs = [7, 8], 16
    cfgd = _cfg()
    env_cfg = kcfg.to_env_config(cfgd)
    route_q = rcfg.load_route_q(GOLDEN / "synthetic_route.json")
    pcfg = PPOConfig(n_steps=64, batch_size=256, n_epochs=2, hidden=64, learning_rate=2e-4, ent_coef=1e-3)
    penv = RoutePopulationVecEnv(env_cfg, rcfg.route_config_from_dict(cfgd, max_route_index=10), route_q, seeds, n_envs)
    pcur = RoutePrefixCurriculumPopulation(**_curriculum_kwargs())
    pop = RoutePopulationPPO(seeds, dataclasses.replace(pcfg), penv, curriculum=pcur, use_graphs=use_graphs)
    pop.load_init_checkpoint(init_checkpoint)
    singles, envs, curs = [], [], []
    for s in seeds:
        env = RouteVecEnv(env_cfg, rcfg.route_config_from_dict(cfgd, max_route_index=10), route_q, n_envs, seed=s)
        cur = RoutePrefixCurriculumDevice(**_curriculum_kwargs())
        p = PPO(env, dataclasses.replace(pcfg, seed=s), curriculum=cur, use_graphs=use_graphs)
        p.load_checkpoint(init_checkpoint, restore_timesteps=True, restore_hyperparameters=True)
        singles.append(p)
        envs.append(env)
        curs.append(cur)
    assert pop.num_timesteps == singles[0].num_timesteps > 0 and pop.adam_t == singles[0].adam_t > 0
    for k, p in enumerate(singles):
        assert torch.equal(p.policy.flat, pop.flat[k]) and torch.equal(p.adam_m, pop.adam_m[k])
    N = n_envs
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
        for k, (p, cur) in enumerate(zip(singles, curs)):
            assert torch.equal(p.policy.flat, pop.flat[k]), (it, k)
            assert torch.equal(p.adam_m, pop.adam_m[k]) and torch.equal(p.adam_v, pop.adam_v[k]), (it, k)
            assert p.adam_t == pop.adam_t and p.num_timesteps == pop.num_timesteps, (it, k)
            assert _tracker_bytes(cur.read()) == _tracker_bytes(pcur.read(k)), (it, k)
            assert cur.summary() == pcur.summary(k) == pop.replica(k).curriculum.summary(), (it, k)
    assert any(pcur.summary(k)["history"] for k in range(len(seeds))), "no replica promoted: the tracker was compared at stage 0 only"
    assert not torch.equal(pop.flat[0], pop.flat[1])
    pop.close()
    pcur.close()
    penv.close()
    for p, cur, env in zip(singles, curs, envs):
        cur.close()
        env.close()


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_train_route_cli_seeds_matches_single_seed_run(tmp_path):
    from rl_brain_trainer_amd import checkpoint as ck
    from rl_brain_trainer_amd import train_route

    cfgd = _cfg()
    cfgd["route"]["curriculum"] = {**cfgd["route"].get("curriculum", {}), "prefix_stages": [10, 20], "promotion_window_episodes": 16,
                                   "min_episodes_per_stage": 16, "promotion_success_rate": 0.0, "promotion_route_ready_hit_rate": 0.0,
                                   "promotion_orientation_hit_rate": 0.0, "promotion_max_regression_rate": 1.0}
    cfgd["route"]["teacher_anchor"] = {"enabled": False}
    cfgd["route"]["sequential_gate"] = {"enabled": True, "prefixes": [5, 10], "full_end_index": 12}
    cfgd["route"]["route_path"] = str(GOLDEN / "synthetic_route.json")
    cfgd["route"].pop("init_checkpoint", None)
    cfgd.setdefault("training", {})["checkpoint_freq"] = 2048
    cfg_path = tmp_path / "route.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgd))
    common = ["--config", str(cfg_path), "--n-envs", "16", "--n-steps", "64", "--batch-size", "256", "--hidden", "64"]
    init = tmp_path / "init"
    train_route.main(common + ["--run-id", "init", "--output-dir", str(init), "--total-timesteps", "1024", "--seed", "3"])
    init_zip = str(init / "model_latest.zip")
    pop_out = tmp_path / "pop"
    summary = train_route.main(common + ["--run-id", "pop", "--output-dir", str(pop_out), "--total-timesteps", "4096", "--seeds", "7,8",
                                         "--init-checkpoint", init_zip])
    single_out = tmp_path / "single7"
    single = train_route.main(common + ["--run-id", "s7", "--output-dir", str(single_out), "--total-timesteps", "4096", "--seed", "7",
                                        "--init-checkpoint", init_zip])
    assert summary["seeds"] == [7, 8] and summary["best_seed"] in (7, 8) and "gate accepted first" in summary["selection"]
    assert (pop_out / "population_summary.json").exists()
    for s in (7, 8):
        root = pop_out / f"seed_{s}"
        for name in ("model_latest.zip", "curriculum_history.json", "training_summary.json", "route_eval_sequential/route_eval_sequential_summary.json",
                     "route_gate/route_gate_summary.json", "checkpoints/model_2048_steps.zip"):
            assert (root / name).exists(), (s, name)
        ts = json.loads((root / "training_summary.json").read_text())
        assert ts["observation_dim"] == 80 and ts["evaluation_wall_seconds"] > 0
        assert ts["route_gate_summary"]["schema_version"] == "v5.route_gate.v1"
        hist = json.loads((root / "curriculum_history.json").read_text())
        assert hist["prefix_end_index"] == 20 and len(hist["history"]) == 1, s     # open thresholds: promoted once
    # seed 7 of the population is the --seed 7 run
    assert json.loads((pop_out / "seed_7" / "curriculum_history.json").read_text()) == json.loads((single_out / "curriculum_history.json").read_text())
    a, b = ck.load_policy_state_dict(pop_out / "seed_7" / "model_latest.zip"), ck.load_policy_state_dict(single_out / "model_latest.zip")
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    oa, ob = ck.load_optimizer_state_dict(pop_out / "seed_7" / "model_latest.zip"), ck.load_optimizer_state_dict(single_out / "model_latest.zip")
    for i in ob["state"]:
        assert torch.equal(oa["state"][i]["exp_avg"], ob["state"][i]["exp_avg"]) and float(oa["state"][i]["step"]) == float(ob["state"][i]["step"])
    assert single["num_timesteps"] == json.loads((pop_out / "seed_7" / "training_summary.json").read_text())["num_timesteps"]
