"""Population PPO on the GPU: replica k of a population handle / PopulationPPO is bit-identical to a single K = 1 run with seed s_k."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("n", [256, 200, 33, 1])
@pytest.mark.parametrize("normalize_mode", [1, 2])
def test_population_kernels_match_single_handles(hidden, n, normalize_mode):
    from rl_brain_trainer_amd import mlp
    from rl_brain_trainer_amd.ppo import ActorCritic

    dev, K, total = _dev(), 3, 1024
    g = torch.Generator(device="cpu").manual_seed(hidden + n)
    pols = [ActorCritic(hidden, dev, seed=11 + k) for k in range(K)]
    for p in pols:   # non-zero biases / log_std so every parameter path carries signal
        p.flat.add_(0.05 * torch.randn(p.numel, generator=g).to(dev))
    P = pols[0].numel
    pop = mlp.MlpKernels(hidden, dev, max_batch=n, replicas=K)
    singles = [mlp.MlpKernels(hidden, dev, max_batch=n) for _ in range(K)]
    assert pop.replicas == K and all(s.replicas == 1 for s in singles)
    flat = torch.stack([p.flat for p in pols]).contiguous()
    pop.pack(flat)
    for s, p in zip(singles, pols):
        s.pack(p.flat)

    # forward: K * n rows, replica-major
    obs = torch.zeros((K * n, 64), device=dev)
    obs[:, :56] = torch.randn((K * n, 56), generator=g).to(dev)
    noise = torch.randn((K * n, 7), generator=g).to(dev)
    outs = {k: torch.empty(shape, device=dev) for k, shape in (("mean", (K * n, 7)), ("value", (K * n,)), ("action", (K * n, 7)),
                                                                  ("clipped", (K * n, 7)), ("log_prob", (K * n,)))}
    pop.forward(obs, noise=noise, **outs)
    for k, s in enumerate(singles):
        r = slice(k * n, (k + 1) * n)
        one = {name: torch.empty_like(t[r]) for name, t in outs.items()}
        s.forward(obs[r].contiguous(), noise=noise[r].contiguous(), **one)
        for name in one:
            assert torch.equal(one[name], outs[name][r]), (name, k)

    # loss_grad + adam_step on shared sample buffers, replica k gathering its own rows
    sobs = torch.zeros((total, 64), device=dev)
    sobs[:, :56] = torch.randn((total, 56), generator=g).to(dev)
    act = torch.randn((total, 7), generator=g).to(dev)
    old_logp = (-8.0 + torch.randn(total, generator=g)).to(dev)
    adv = torch.randn(total, generator=g).to(dev)
    ret = torch.randn(total, generator=g).to(dev)
    idx = torch.stack([torch.randperm(total, generator=g)[:n] for _ in range(K)]).to(dev).contiguous()
    adv_stats = None
    if normalize_mode == 2:
        a = adv[idx]
        std = a.std(1) if n > 1 else torch.zeros(K, device=a.device)     # one row: the kernels' own definition, 1 / (0 + 1e-8)
        adv_stats = torch.stack([a.mean(1), 1.0 / (std + 1e-8)], dim=1).float().contiguous()      # [K][2]
    kw = dict(clip_range=0.2, ent_coef=1e-3, vf_coef=0.5, inv_count=1.0 / n)
    grad = torch.zeros((K, P), device=dev)
    stats = torch.zeros((K, 4), device=dev)
    m, v = torch.zeros_like(grad), torch.zeros_like(grad)
    params = flat.clone()
    pop.set_step_count(0)
    for _ in range(2):   # two steps: the moments and the shared step count carry over
        pop.loss_grad(sobs, idx, n, act, old_logp, adv, ret, grad_out=grad, stats_out=stats, adv_stats=adv_stats, **kw)
        pop.adam_step(params, grad, m, v, lr=3e-4, eps=1e-5, max_grad_norm=0.5, step=0, fused_norm=True)
    for k, s in enumerate(singles):
        gk, sk = torch.zeros(P, device=dev), torch.zeros(4, device=dev)
        pk, mk, vk = flat[k].clone(), torch.zeros(P, device=dev), torch.zeros(P, device=dev)
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


# ---------------------------------------------------------------------------------------------------------------- trainer level
def _approach(n_envs=16, n_steps=64, batch=256):
    from rl_brain_trainer_amd import config as kcfg
    from rl_brain_trainer_amd.curriculum import PointCurriculum
    from rl_brain_trainer_amd.ppo import PPOConfig
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    cfg = kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml")
    env_cfg = kcfg.to_env_config(cfg)
    assert env_cfg.c.curriculum_enabled and env_cfg.n_stages

    def env_factory(seed):
        return ArmKinematicVecEnv(env_cfg, n_envs, seed=seed)

    def cur_factory(seed):
        # threshold 0 and a small window: promotions happen inside the few iterations of the test
        return PointCurriculum(success_rate_threshold=0.0, window_episodes=4,
                               min_episodes_per_stage=4, max_stage_index=env_cfg.n_stages - 1)

    pcfg = PPOConfig(n_steps=n_steps, batch_size=batch, n_epochs=3, hidden=64, learning_rate=3e-4, ent_coef=1e-3)
    return pcfg, env_factory, cur_factory


def _dock(n_envs=16, n_steps=64, batch=256):
    from rl_brain_trainer_amd import config as kcfg
    from rl_brain_trainer_amd.finisher_tools import DockReverseCurriculum
    from rl_brain_trainer_amd.ppo import PPOConfig
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    dock = kcfg.load_yaml_file(kcfg.builtin_config_dir() / "dock_workspace_handoff_noop_ft_12env.yaml")
    dock["env"]["dock_reset"]["handoff_state_probability"] = 0.0
    env_cfg = kcfg.to_env_config(dock)
    stages = [{"name": "anchor", "min_episodes": 4, "window_episodes": 4, "success_rate_threshold": 0.0, "dock_residual_action_limit": 0.2},
              {"name": "wide", "close_bucket_probability": 0.2, "dock_residual_action_limit": 0.35}]

    def env_factory(seed):
        return ArmKinematicVecEnv(env_cfg, n_envs, seed=seed)

    def cur_factory(seed):
        return DockReverseCurriculum(stages=stages, window_episodes=4)

    pcfg = PPOConfig(n_steps=n_steps, batch_size=batch, n_epochs=2, hidden=64, learning_rate=3e-4)
    return pcfg, env_factory, cur_factory


def _tracker_state(cur):
    import ctypes as C

    st = cur.read()
    return bytes(C.string_at(C.addressof(st), C.sizeof(st)))


BUFFERS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf")


def _run_and_compare(setup, seeds, iters, use_graphs):
    import dataclasses

    from rl_brain_trainer_amd.population import PopulationPPO
    from rl_brain_trainer_amd.ppo import PPO

    pcfg, env_factory, cur_factory = setup()
    pop = PopulationPPO(seeds, pcfg, env_factory, curriculum_factory=cur_factory, use_graphs=use_graphs)
    singles = []
    for s in seeds:
        singles.append(PPO(env_factory(s), dataclasses.replace(pcfg, seed=s), curriculum=cur_factory(s), use_graphs=use_graphs))
    N = pop.n_envs
    for _ in range(iters):
        pop.collect_rollouts()
        for p in singles:
            p.collect_rollouts()
        torch.cuda.synchronize()
        for k, p in enumerate(singles):
            sl = slice(k * N, (k + 1) * N)
            for name in BUFFERS:
                a, b = getattr(p, name), getattr(pop, name)[:, sl]
                assert torch.equal(a, b), (name, k)
        pop.train()
        for p in singles:
            p.train()
        torch.cuda.synchronize()
        for k, p in enumerate(singles):
            assert torch.equal(p.policy.flat, pop.flat[k]), k
            assert torch.equal(p.adam_m, pop.adam_m[k]) and torch.equal(p.adam_v, pop.adam_v[k]), k
            assert p.adam_t == pop.adam_t and p.num_timesteps == pop.num_timesteps
            assert _tracker_state(p.curriculum) == _tracker_state(pop.curricula[k]), k
            assert p.last_stats == pop.replica(k).last_stats, k
    return pop, singles


def _close(pop, singles):
    pop.close()
    for p in singles:
        p.env.close()


@pytest.mark.parametrize("use_graphs", [True, False])
def test_population_ppo_bit_identical_to_single_runs(use_graphs):
    pop, singles = _run_and_compare(_approach, [7, 8, 9], 3, use_graphs)
    stages = [pop.curricula[k].read().stage_index for k in range(3)]
    assert max(stages) > 0, "the test's curriculum never promoted: tracker state compared only at stage 0"
    assert not torch.equal(pop.flat[0], pop.flat[1])
    _close(pop, singles)


@pytest.mark.parametrize("use_graphs", [True, False])
def test_population_ppo_dock_reverse_curriculum(use_graphs):
    pop, singles = _run_and_compare(_dock, [3, 4], 2, use_graphs)
    _close(pop, singles)


def test_population_ppo_ragged_last_minibatch():
    """1024 rows per replica in minibatches of 192: five full ones and a ragged 64-row tail, in the rows -> [K][n] index mapping too"""
    pop, singles = _run_and_compare(lambda: _approach(batch=192), [7, 8], 2, True)
    assert pop._mb[-1] == (960, 1024)
    _close(pop, singles)


def test_population_of_one_equals_ppo():
    pop, singles = _run_and_compare(_approach, [5], 2, True)
    _close(pop, singles)


def test_population_checkpoint_hand_over(tmp_path):
    """replica 1 saved as an ordinary archive and loaded into a single PPO continues bit-identically to the population"""
    import dataclasses

    from rl_brain_trainer_amd import checkpoint
    from rl_brain_trainer_amd.population import PopulationPPO
    from rl_brain_trainer_amd.ppo import PPO, InferencePolicy

    pcfg, env_factory, _ = _approach()
    seeds = [7, 8]
    pop = PopulationPPO(seeds, pcfg, env_factory, use_graphs=True)
    pop.collect_rollouts()
    pop.train()
    path = checkpoint.save(tmp_path / "replica1", pop.replica(1))
    sd = checkpoint.load_policy_state_dict(path)
    assert all(torch.equal(sd[k_].to(pop.device), v) for k_, v in pop.policies[1].views.items())
    obs = torch.zeros((32, 64), device=pop.device)
    obs[:, :56] = torch.randn((32, 56), device=pop.device)
    assert torch.equal(InferencePolicy.load(str(path)).predict(obs), pop.replica(1).predict(obs))
    # what acts on one policy is refused on the population handle itself: it points to replica(k) / infer_policy(k)
    for single_policy_call in (lambda: pop.predict(obs), lambda: pop.predict_unclipped(obs), lambda: pop.load_checkpoint(str(path)),
                               lambda: pop.last_stats):
        with pytest.raises(TypeError, match=r"replica\(k\).*infer_policy\(k\)"):
            single_policy_call()

    # a single run with the same seed is at the same point in its streams once it has done the same iteration; then it takes the archive
    single = PPO(env_factory(8), dataclasses.replace(pcfg, seed=8), use_graphs=True)
    single.collect_rollouts()
    single.train()
    single.policy.flat.zero_()
    single.adam_m.zero_()
    single.adam_v.zero_()
    single.load_checkpoint(str(path))
    assert single.adam_t == pop.adam_t
    pop.collect_rollouts()
    pop.train()
    single.collect_rollouts()
    single.train()
    torch.cuda.synchronize()
    assert torch.equal(single.policy.flat, pop.flat[1])
    assert torch.equal(single.adam_m, pop.adam_m[1]) and torch.equal(single.adam_v, pop.adam_v[1])
    pop.close()
    single.env.close()


def test_train_cli_seeds_matches_single_seed_runs(tmp_path):
    """train.py --seeds 7,8 leaves seed_7/ and seed_8/ whose policies equal those of train.py --seed 7 / --seed 8, and a population summary"""
    import json

    import yaml

    from rl_brain_trainer_amd import checkpoint, config as kcfg, train

    overlay = {"base_config": str(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"),
               "workspace_expansion": {"init_approach_checkpoint": "", "finisher_checkpoint": ""}}
    cfg_path = tmp_path / "run.yaml"
    cfg_path.write_text(yaml.safe_dump(overlay))
    common = ["--config", str(cfg_path), "--total-timesteps", "2048", "--n-envs", "16", "--n-steps", "64", "--batch-size", "256", "--hidden", "64",
              "--log-every", "0"]
    pop_root = tmp_path / "pop"
    summary = train.main(common + ["--run-id", "p", "--artifact-root", str(pop_root), "--seeds", "7,8"])
    on_disk = json.loads((pop_root / "population_summary.json").read_text())
    assert on_disk["seeds"] == [7, 8] and on_disk["replicas"] == 2 and on_disk["num_timesteps_per_seed"] == 2048
    assert [r["seed"] for r in on_disk["per_seed"]] == [7, 8] and on_disk["aggregate_env_steps_per_second"] > 0
    assert on_disk["best_seed"] is None     # no gate ran: no selection
    assert summary["per_seed"][0]["model_latest"] == on_disk["per_seed"][0]["model_latest"]
    for s in (7, 8):
        d = pop_root / f"seed_{s}"
        for name in ("model_latest.zip", "latest_checkpoint/model_latest.zip", "config_resolved.yaml", "training_launch_summary.json", "training_summary.json"):
            assert (d / name).exists(), (s, name)
        ts = json.loads((d / "training_summary.json").read_text())
        assert ts["seed"] == s and ts["num_timesteps"] == 2048
        single_root = tmp_path / f"single_{s}"
        train.main(common + ["--run-id", f"s{s}", "--artifact-root", str(single_root), "--seed", str(s)])
        a = checkpoint.load_policy_state_dict(d / "model_latest.zip")
        b = checkpoint.load_policy_state_dict(single_root / "model_latest.zip")
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), s
    a7 = checkpoint.load_policy_state_dict(pop_root / "seed_7" / "model_latest.zip")
    a8 = checkpoint.load_policy_state_dict(pop_root / "seed_8" / "model_latest.zip")
    assert not torch.equal(a7["action_net.weight"], a8["action_net.weight"])


def test_train_dock_cli_seeds(tmp_path):
    """train_dock.py --seeds 3,4: per-seed Finisher artefacts, seed 3's policy equal to that of --seed 3, and the dock-eval selection"""
    import json

    import yaml

    from rl_brain_trainer_amd import checkpoint, config as kcfg, train_dock

    dock = kcfg.load_yaml_file(kcfg.builtin_config_dir() / "dock_workspace_handoff_noop_ft_12env.yaml")
    dock["env"]["dock_reset"]["handoff_state_probability"] = 0.0           # the reference's handoff buffer file is not shipped
    dock.setdefault("training", {})["dock_reverse_curriculum"] = {
        "enabled": True, "window_episodes": 8,
        "stages": [{"name": "anchor", "min_episodes": 8, "window_episodes": 8, "success_rate_threshold": 0.0, "dock_residual_action_limit": 0.2},
                   {"name": "wide", "close_bucket_probability": 0.2, "dock_residual_action_limit": 0.35}]}
    cfg_path = tmp_path / "dock.yaml"
    cfg_path.write_text(yaml.safe_dump(dock))
    common = ["--config", str(cfg_path), "--total-timesteps", "2048", "--n-envs", "16", "--n-steps", "64", "--batch-size", "256", "--hidden", "64",
              "--eval-episodes", "16", "--log-every", "0"]
    root = tmp_path / "pop"
    summary = train_dock.main(common + ["--run-id", "p", "--artifact-root", str(root), "--seeds", "3,4"])
    on_disk = json.loads((root / "population_summary.json").read_text())
    assert on_disk["seeds"] == [3, 4] and on_disk["best_seed"] in (3, 4) and summary["best_seed"] == on_disk["best_seed"]
    for s in (3, 4):
        for name in ("model_latest.zip", "dock_eval/dock_eval_summary.json", "training_summary.json"):
            assert (root / f"seed_{s}" / name).exists(), (s, name)
    single = tmp_path / "single"
    train_dock.main(common + ["--run-id", "s", "--artifact-root", str(single), "--seed", "3"])
    a = checkpoint.load_policy_state_dict(root / "seed_3" / "model_latest.zip")
    b = checkpoint.load_policy_state_dict(single / "model_latest.zip")
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert (json.loads((single / "dock_eval" / "dock_eval_summary.json").read_text())
            == json.loads((root / "seed_3" / "dock_eval" / "dock_eval_summary.json").read_text()))
