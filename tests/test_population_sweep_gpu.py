"""Per-replica PPO hyper-parameters on the GPU: replica k of a population handle with hyper-parameter table entry h computes bit for bit what a
K = 1 handle computes with h's scalars; kp1_gae_scan_replicas equals K single scans; Approach, route and dock populations with overrides equal
single PPO(cfg_k) runs; `--sweep` replicas and `train.py --seeds --resume-from` equal the matching --seed runs."""
from __future__ import annotations

import ctypes as C
import dataclasses
import json

import pytest
import torch
import yaml

from conftest import GOLDEN
from rl_brain_trainer_amd import config as kcfg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FIELDS = ("learning_rate", "adam_eps", "max_grad_norm", "clip_range", "ent_coef", "vf_coef")
# entry 0 clips the gradient norm hard, entry 1 clips the ratio tightly, entry 2 has its own entropy / value weights
TABLE = [dict(learning_rate=3e-4, adam_eps=1e-5, max_grad_norm=1e-3, clip_range=0.2, ent_coef=1e-3, vf_coef=0.5),
         dict(learning_rate=1e-3, adam_eps=1e-6, max_grad_norm=0.5, clip_range=0.01, ent_coef=0.0, vf_coef=0.25),
         dict(learning_rate=5e-5, adam_eps=1e-4, max_grad_norm=2.0, clip_range=0.3, ent_coef=0.05, vf_coef=1.0)]


# ---------------------------------------------------------------------------------------------------------------- kernels
def _train_pop(mk, table, flat, sobs, idx, n, act, old_logp, adv, ret, scalars):
    K, P = flat.shape
    grad, stats = torch.zeros((K, P), device=DEV), torch.zeros((K, 4), device=DEV)
    m, v, params = torch.zeros_like(grad), torch.zeros_like(grad), flat.clone()
    mk.set_replica_hparams(table)
    mk.set_step_count(0)
    for _ in range(2):
        mk.loss_grad(sobs, idx, n, act, old_logp, adv, ret, clip_range=scalars["clip_range"], ent_coef=scalars["ent_coef"],
                     vf_coef=scalars["vf_coef"], inv_count=1.0 / n, grad_out=grad, stats_out=stats)
        mk.adam_step(params, grad, m, v, lr=scalars["learning_rate"], eps=scalars["adam_eps"], max_grad_norm=scalars["max_grad_norm"], step=0,
                     fused_norm=True)
    torch.cuda.synchronize()
    return {"grad": grad, "stats": stats, "params": params, "m": m, "v": v}


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("obs_dim", [56, 80])
def test_replica_table_matches_single_handles(hidden, obs_dim):
    """K = 3 handle with three distinct entries against three K = 1 handles called with the matching scalars: forward, two loss_grad + Adam
    steps (grad, stats, params, m, v) bitwise; clipping of the gradient norm and of the ratio both engage"""
    from rl_brain_trainer_amd import mlp
    from rl_brain_trainer_amd.ppo import ActorCritic

    K, n, total = len(TABLE), 256, 1024
    width = 64 if obs_dim == 56 else 128
    g = torch.Generator(device="cpu").manual_seed(hidden + obs_dim)
    pols = [ActorCritic(hidden, DEV, seed=21 + k, obs_dim=obs_dim) for k in range(K)]
    for p in pols:
        p.flat.add_(0.05 * torch.randn(p.numel, generator=g).to(DEV))
    P = pols[0].numel
    flat = torch.stack([p.flat for p in pols]).contiguous()
    pop = mlp.MlpKernels(hidden, DEV, max_batch=n, obs_dim=obs_dim, replicas=K)
    pop.pack(flat)
    obs = torch.zeros((K * n, width), device=DEV)
    obs[:, :obs_dim] = torch.randn((K * n, obs_dim), generator=g).to(DEV)
    noise = torch.randn((K * n, 7), generator=g).to(DEV)
    mean, value = torch.empty((K * n, 7), device=DEV), torch.empty(K * n, device=DEV)
    pop.set_replica_hparams(TABLE)
    pop.forward(obs, noise=noise, mean=mean, value=value)
    sobs = torch.zeros((total, width), device=DEV)
    sobs[:, :obs_dim] = torch.randn((total, obs_dim), generator=g).to(DEV)
    act = torch.randn((total, 7), generator=g).to(DEV)
    old_logp = (-8.0 + torch.randn(total, generator=g)).to(DEV)
    adv = torch.randn(total, generator=g).to(DEV)
    ret = torch.randn(total, generator=g).to(DEV)
    idx = torch.stack([torch.randperm(total, generator=g)[:n] for _ in range(K)]).to(DEV).contiguous()
    # the shared scalars are deliberately none of the entries: with a table they must be ignored
    shared = dict(learning_rate=0.1, adam_eps=0.5, max_grad_norm=100.0, clip_range=0.9, ent_coef=0.7, vf_coef=3.0)
    out = _train_pop(pop, TABLE, flat, sobs, idx, n, act, old_logp, adv, ret, shared)
    for k, h in enumerate(TABLE):
        one = mlp.MlpKernels(hidden, DEV, max_batch=n, obs_dim=obs_dim)
        one.pack(flat[k].contiguous())
        r = slice(k * n, (k + 1) * n)
        m1, v1 = torch.empty((n, 7), device=DEV), torch.empty(n, device=DEV)
        one.forward(obs[r].contiguous(), noise=noise[r].contiguous(), mean=m1, value=v1)
        assert torch.equal(m1, mean[r]) and torch.equal(v1, value[r]), k
        gk, sk = torch.zeros(P, device=DEV), torch.zeros(4, device=DEV)
        pk, mk_, vk = flat[k].clone(), torch.zeros(P, device=DEV), torch.zeros(P, device=DEV)
        one.set_step_count(0)
        for _ in range(2):
            one.loss_grad(sobs, idx[k].contiguous(), n, act, old_logp, adv, ret, clip_range=h["clip_range"], ent_coef=h["ent_coef"],
                          vf_coef=h["vf_coef"], inv_count=1.0 / n, grad_out=gk, stats_out=sk)
            one.adam_step(pk, gk, mk_, vk, lr=h["learning_rate"], eps=h["adam_eps"], max_grad_norm=h["max_grad_norm"], step=0, fused_norm=True)
        torch.cuda.synchronize()
        for name, a in (("grad", gk), ("stats", sk), ("params", pk), ("m", mk_), ("v", vk)):
            assert torch.equal(a, out[name][k]), (name, k)
        one.close()
    # entry 0's max_grad_norm is far below its gradient's norm: clip_grad_norm_ engaged
    assert float(out["grad"][0].double().norm()) > 10 * TABLE[0]["max_grad_norm"]
    with pytest.raises(ValueError):
        pop.set_replica_hparams(TABLE[:2])
    pop.close()


def test_uniform_table_equals_no_table():
    """a table whose every entry holds the scalars computes bit for bit what the handle computes without a table; a K = 1 handle refuses one"""
    from rl_brain_trainer_amd import mlp, native
    from rl_brain_trainer_amd.ppo import ActorCritic

    K, n, total, hidden = 4, 200, 800, 64
    g = torch.Generator(device="cpu").manual_seed(5)
    flat = torch.stack([ActorCritic(hidden, DEV, seed=3 + k).flat for k in range(K)]).contiguous()
    sobs = torch.zeros((total, 64), device=DEV)
    sobs[:, :56] = torch.randn((total, 56), generator=g).to(DEV)
    act = torch.randn((total, 7), generator=g).to(DEV)
    old_logp = (-8.0 + torch.randn(total, generator=g)).to(DEV)
    adv, ret = torch.randn(total, generator=g).to(DEV), torch.randn(total, generator=g).to(DEV)
    idx = torch.stack([torch.randperm(total, generator=g)[:n] for _ in range(K)]).to(DEV).contiguous()
    scalars = TABLE[0]
    pop = mlp.MlpKernels(hidden, DEV, max_batch=n, replicas=K)
    pop.pack(flat)
    with_table = _train_pop(pop, [scalars] * K, flat, sobs, idx, n, act, old_logp, adv, ret, scalars)
    pop.pack(flat)
    without = _train_pop(pop, None, flat, sobs, idx, n, act, old_logp, adv, ret, scalars)
    for name in with_table:
        assert torch.equal(with_table[name], without[name]), name
    pop.close()
    one = mlp.MlpKernels(hidden, DEV, max_batch=n)
    with pytest.raises(native.Kp1Error):
        one.set_replica_hparams([scalars])
    one.set_replica_hparams(None)
    one.close()


def test_gae_scan_replicas_matches_single_scans():
    """kp1_gae_scan_replicas against K kp1_gae_scan calls on the replicas' columns, terminated and truncated dones, bitwise"""
    from rl_brain_trainer_amd import native

    L = native.load()
    T, N, K = 96, 40, 3
    gl = [(0.99, 0.95), (0.95, 0.9), (0.999, 0.8)]
    g = torch.Generator(device="cpu").manual_seed(9)
    rew, val = torch.randn((T, K * N), generator=g).to(DEV), torch.randn((T, K * N), generator=g).to(DEV)
    last = torch.randn(K * N, generator=g).to(DEV)
    u = torch.rand((T, K * N), generator=g)
    done = torch.where(u < 0.05, 1, torch.where(u < 0.1, 2, torch.where(u < 0.12, 3, 0))).to(torch.uint8).to(DEV)   # KP1_DONE_* bits
    table = torch.tensor(gl, dtype=torch.float32, device=DEV)
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    native.check(L.kp1_gae_scan_replicas(0, p(rew), p(val), p(done), p(last), p(table), N, p(adv), p(ret), T, K * N, s))
    for k, (gamma, lam) in enumerate(gl):
        sl = slice(k * N, (k + 1) * N)
        r, v, d = (x[:, sl].contiguous() for x in (rew, val, done))
        lv = last[sl].contiguous()
        a1, r1 = torch.empty_like(r), torch.empty_like(r)
        native.check(L.kp1_gae_scan(0, p(r), p(v), p(d), p(lv), gamma, lam, p(a1), p(r1), T, N, s))
        torch.cuda.synchronize()
        assert torch.equal(a1, adv[:, sl]) and torch.equal(r1, ret[:, sl]), k


# ---------------------------------------------------------------------------------------------------------------- trainers
BUFFERS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf", "term_obs_buf")
# replicas 0 and 1 share seed 7 and differ in the learning rate; replica 2 discounts differently and clips tighter
SEEDS = [7, 7, 8]
OVERRIDES = [{"learning_rate": 3e-4}, {"learning_rate": 1e-4, "ent_coef": 1e-2}, {"gamma": 0.95, "gae_lambda": 0.9, "clip_range": 0.1,
                                                                                  "max_grad_norm": 0.05}]


def _tracker_bytes(st) -> bytes:
    return bytes(C.string_at(C.addressof(st), C.sizeof(st)))


def _compare(pop, singles, read_tracker, iters=3):
    N = pop.n_envs
    first = None
    for it in range(iters):
        pop.collect_rollouts()
        for p in singles:
            p.collect_rollouts()
        torch.cuda.synchronize()
        for k, p in enumerate(singles):
            sl = slice(k * N, (k + 1) * N)
            for name in BUFFERS:
                assert torch.equal(getattr(p, name), getattr(pop, name)[:, sl]), (it, name, k)
        if it == 0:
            first = pop.act_buf.clone()
            assert torch.equal(first[:, :N], first[:, N:2 * N]), "two replicas on one seed must share their first rollout"
        pop.train()
        for p in singles:
            p.train()
        torch.cuda.synchronize()
        for k, p in enumerate(singles):
            assert torch.equal(p.policy.flat, pop.flat[k]), (it, k)
            assert torch.equal(p.adam_m, pop.adam_m[k]) and torch.equal(p.adam_v, pop.adam_v[k]), (it, k)
            assert p.adam_t == pop.adam_t and p.num_timesteps == pop.num_timesteps, (it, k)
            assert p.last_stats == pop.replica(k).last_stats, (it, k)
            if read_tracker is not None:
                assert _tracker_bytes(p.curriculum.read()) == _tracker_bytes(read_tracker(k)), (it, k)
            assert pop.replica(k).cfg == p.cfg, k
    assert not torch.equal(pop.flat[0], pop.flat[1]), "the same-seed replicas must differ after an update"


@pytest.mark.parametrize("use_graphs", [True, False])
def test_approach_population_overrides_match_single_runs(use_graphs):
    from rl_brain_trainer_amd.curriculum import PointCurriculum, PointCurriculumPopulation
    from rl_brain_trainer_amd.population import ApproachPopulationPPO
    from rl_brain_trainer_amd.ppo import PPO, PPOConfig
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    env_cfg = kcfg.to_env_config(kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"))
    N = 16
    kw = {"success_rate_threshold": 0.0, "window_episodes": 4, "min_episodes_per_stage": 4, "max_stage_index": env_cfg.n_stages - 1}
    pcfg = PPOConfig(n_steps=64, batch_size=256, n_epochs=3, hidden=64, learning_rate=3e-4, ent_coef=1e-3)
    penv = ArmKinematicPopulationVecEnv(env_cfg, SEEDS, N, repeated_seeds=True)
    pcur = PointCurriculumPopulation(**kw, initial_stage_indices=[0, 0, 2])
    pop = ApproachPopulationPPO(SEEDS, dataclasses.replace(pcfg), penv, curriculum=pcur, use_graphs=use_graphs, overrides=OVERRIDES)
    singles = [PPO(ArmKinematicVecEnv(env_cfg, N, seed=s), dataclasses.replace(pcfg, seed=s, **o), curriculum=PointCurriculum(**kw, initial_stage_index=st),
                   use_graphs=use_graphs) for s, o, st in zip(SEEDS, OVERRIDES, [0, 0, 2])]
    _compare(pop, singles, pcur.read)
    pop.close()
    pcur.close()
    penv.close()
    for p in singles:
        p.curriculum.close()
        p.env.close()


@pytest.mark.parametrize("use_graphs", [True, False])
def test_dock_population_overrides_match_single_runs(use_graphs):
    from rl_brain_trainer_amd import finisher_tools as ft
    from rl_brain_trainer_amd.population import DockPopulationPPO
    from rl_brain_trainer_amd.ppo import PPO, PPOConfig
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    dock = kcfg.load_yaml_file(kcfg.builtin_config_dir() / "dock_workspace_handoff_noop_ft_12env.yaml")
    dock["env"]["dock_reset"]["handoff_state_probability"] = 0.0
    env_cfg = kcfg.to_env_config(dock)
    stages = [{"name": "anchor", "min_episodes": 4, "window_episodes": 4, "success_rate_threshold": 0.0, "dock_residual_action_limit": 0.2},
              {"name": "wide", "close_bucket_probability": 0.2, "dock_residual_action_limit": 0.35}]
    N = 12
    pcfg = PPOConfig(n_steps=64, batch_size=128, n_epochs=2, hidden=64, learning_rate=3e-4, ent_coef=1e-3)
    penv = ArmKinematicPopulationVecEnv(env_cfg, SEEDS, N, mode="dock", repeated_seeds=True)
    pcur = ft.DockReverseCurriculumPopulation(stages=stages, window_episodes=4, n_replicas=len(SEEDS))
    pop = DockPopulationPPO(SEEDS, dataclasses.replace(pcfg), penv, curriculum=pcur, use_graphs=use_graphs, overrides=OVERRIDES)
    singles = [PPO(ArmKinematicVecEnv(kcfg.to_env_config(dock), N, seed=s), dataclasses.replace(pcfg, seed=s, **o),
                   curriculum=ft.DockReverseCurriculum(stages=stages, window_episodes=4), use_graphs=use_graphs) for s, o in zip(SEEDS, OVERRIDES)]
    _compare(pop, singles, None)
    for k, p in enumerate(singles):
        assert _tracker_bytes(p.curriculum.read()) == _tracker_bytes(pcur.read(k)), k
    pop.close()
    pcur.close()
    penv.close()
    for p in singles:
        p.curriculum.close()
        p.env.close()


@pytest.mark.parametrize("use_graphs", [True, False])
def test_route_population_overrides_match_single_runs(use_graphs):
    from rl_brain_trainer_amd import route_config as rcfg
    from rl_brain_trainer_amd.population import RoutePopulationPPO
    from rl_brain_trainer_amd.ppo import PPO, PPOConfig
    from rl_brain_trainer_amd.route_curriculum import RoutePrefixCurriculumDevice, RoutePrefixCurriculumPopulation, build_prefix_stages
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv, RouteVecEnv

    cfgd = json.loads((GOLDEN / "configs" / "route_curriculum_prefix120_routeobs_sequence2.json").read_text())
    env_cfg = kcfg.to_env_config(cfgd)
    route_q = rcfg.load_route_q(GOLDEN / "synthetic_route.json")
    kw = dict(stages=build_prefix_stages([10, 20, 30]), promotion_success_rate=0.0, promotion_route_ready_hit_rate=0.0,
              promotion_orientation_hit_rate=0.0, promotion_max_regression_rate=1.0, window_episodes=16, min_episodes_per_stage=16)
    N = 16
    pcfg = PPOConfig(n_steps=64, batch_size=256, n_epochs=2, hidden=64, learning_rate=2e-4, ent_coef=1e-3)
    penv = RoutePopulationVecEnv(env_cfg, rcfg.route_config_from_dict(cfgd, max_route_index=10), route_q, SEEDS, N)
    pcur = RoutePrefixCurriculumPopulation(**kw)
    pop = RoutePopulationPPO(SEEDS, dataclasses.replace(pcfg), penv, curriculum=pcur, use_graphs=use_graphs, overrides=OVERRIDES)
    singles, curs = [], []
    for s, o in zip(SEEDS, OVERRIDES):
        cur = RoutePrefixCurriculumDevice(**kw)
        env = RouteVecEnv(env_cfg, rcfg.route_config_from_dict(cfgd, max_route_index=10), route_q, N, seed=s)
        singles.append(PPO(env, dataclasses.replace(pcfg, seed=s, **o), curriculum=cur, use_graphs=use_graphs))
        curs.append(cur)
    _compare(pop, singles, pcur.read)
    pop.close()
    pcur.close()
    penv.close()
    for p, cur in zip(singles, curs):
        cur.close()
        p.env.close()


# ---------------------------------------------------------------------------------------------------------------- CLI
def _assert_same_zip(a_zip, b_zip, what):
    from rl_brain_trainer_amd import checkpoint

    a, b = checkpoint.load_policy_state_dict(a_zip), checkpoint.load_policy_state_dict(b_zip)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), what
    oa, ob = checkpoint.load_optimizer_state_dict(a_zip), checkpoint.load_optimizer_state_dict(b_zip)
    assert oa["param_groups"] == ob["param_groups"], what
    for i, st in ob["state"].items():
        for name, v in st.items():
            assert torch.equal(torch.as_tensor(oa["state"][i][name]), torch.as_tensor(v)), (what, i, name)
    da, db = checkpoint.load_data(a_zip), checkpoint.load_data(b_zip)
    for key in ("learning_rate", "gamma", "gae_lambda", "clip_range", "ent_coef", "num_timesteps", "seed"):
        assert da.get(key) == db.get(key), (what, key)


def _approach_yaml(tmp_path):
    overlay = {"base_config": str(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"),
               "workspace_expansion": {"init_approach_checkpoint": "", "finisher_checkpoint": ""}}
    cfg_path = tmp_path / "run.yaml"
    cfg_path.write_text(yaml.safe_dump(overlay))
    return ["--config", str(cfg_path), "--total-timesteps", "2048", "--n-envs", "16", "--n-steps", "64", "--batch-size", "256", "--hidden", "64",
            "--log-every", "0"]


def test_train_cli_sweep_matches_single_runs(tmp_path):
    """train.py --seeds 7,8 --sweep learning_rate=1e-4,3e-4: each replica's model_latest.zip (policy, optimiser state, saved learning rate)
    equals train.py --seed s --learning-rate v; population_summary.json names replica and overrides"""
    from rl_brain_trainer_amd import checkpoint, train

    common = _approach_yaml(tmp_path)
    root = tmp_path / "pop"
    summary = train.main(common + ["--run-id", "p", "--artifact-root", str(root), "--seeds", "7,8", "--sweep", "learning_rate=1e-4,3e-4"])
    on_disk = json.loads((root / "population_summary.json").read_text())
    assert on_disk["seeds"] == [7, 7, 8, 8] and summary["replicas"] == 4
    assert [r["replica"] for r in on_disk["per_seed"]] == ["seed_7_learning_rate_0.0001", "seed_7_learning_rate_0.0003",
                                                           "seed_8_learning_rate_0.0001", "seed_8_learning_rate_0.0003"]
    assert [r["overrides"] for r in on_disk["per_seed"]] == [{"learning_rate": v} for _ in (7, 8) for v in (1e-4, 3e-4)]
    assert "best_overrides" in on_disk
    for s in (7, 8):
        for v in ("0.0001", "0.0003"):
            single = tmp_path / f"single_{s}_{v}"
            train.main(common + ["--run-id", f"s{s}", "--artifact-root", str(single), "--seed", str(s), "--learning-rate", v])
            a_zip = root / f"seed_{s}_learning_rate_{v}" / "model_latest.zip"
            _assert_same_zip(a_zip, single / "model_latest.zip", (s, v))
            assert checkpoint.load_data(a_zip)["learning_rate"] == float(v)
            assert checkpoint.load_optimizer_state_dict(a_zip)["param_groups"][0]["lr"] == float(v)


def test_train_cli_seeds_resume_matches_single_runs(tmp_path):
    """train.py --seeds 7,8 --resume-from <zip> against train.py --seed s --resume-from <zip>"""
    from rl_brain_trainer_amd import train

    common = _approach_yaml(tmp_path)
    start = tmp_path / "start"
    train.main(common + ["--run-id", "start", "--artifact-root", str(start), "--seed", "3"])
    zip_path = str(start / "model_latest.zip")
    root = tmp_path / "pop"
    train.main(common + ["--run-id", "p", "--artifact-root", str(root), "--seeds", "7,8", "--resume-from", zip_path])
    for s in (7, 8):
        single = tmp_path / f"single_{s}"
        train.main(common + ["--run-id", f"s{s}", "--artifact-root", str(single), "--seed", str(s), "--resume-from", zip_path])
        _assert_same_zip(root / f"seed_{s}" / "model_latest.zip", single / "model_latest.zip", s)


def test_train_dock_cli_sweep_matches_single_runs(tmp_path):
    """train_dock.py --seeds 3 --sweep learning_rate=1e-4,3e-4 on a temporary YAML against the two --seed 3 --learning-rate v runs"""
    from rl_brain_trainer_amd import train_dock

    dock = kcfg.load_yaml_file(kcfg.builtin_config_dir() / "dock_workspace_handoff_noop_ft_12env.yaml")
    dock["env"]["dock_reset"]["handoff_state_probability"] = 0.0
    dock.setdefault("training", {})["dock_reverse_curriculum"] = {
        "enabled": True, "window_episodes": 8,
        "stages": [{"name": "anchor", "min_episodes": 8, "window_episodes": 8, "success_rate_threshold": 0.0, "dock_residual_action_limit": 0.2},
                   {"name": "wide", "close_bucket_probability": 0.2, "dock_residual_action_limit": 0.35}]}
    cfg_path = tmp_path / "dock.yaml"
    cfg_path.write_text(yaml.safe_dump(dock))
    common = ["--config", str(cfg_path), "--total-timesteps", "2048", "--n-envs", "16", "--n-steps", "64", "--batch-size", "256", "--hidden", "64",
              "--eval-episodes", "16", "--log-every", "0"]
    root = tmp_path / "pop"
    train_dock.main(common + ["--run-id", "p", "--artifact-root", str(root), "--seeds", "3", "--sweep", "learning_rate=1e-4,3e-4"])
    for v in ("0.0001", "0.0003"):
        single = tmp_path / f"single_{v}"
        train_dock.main(common + ["--run-id", "s", "--artifact-root", str(single), "--seed", "3"] + _dock_lr_args(tmp_path, dock, v))
        rep = root / f"seed_3_learning_rate_{v}"
        _assert_same_zip(rep / "model_latest.zip", single / "model_latest.zip", v)
        assert (json.loads((single / "dock_eval" / "dock_eval_summary.json").read_text())
                == json.loads((rep / "dock_eval" / "dock_eval_summary.json").read_text()))


def _dock_lr_args(tmp_path, dock: dict, lr: str) -> list[str]:
    """a --seed run with learning rate `lr`: the dock trainer takes it from the YAML's PPO block"""
    from rl_brain_trainer_amd import train_dock

    if any(a.option_strings == ["--learning-rate"] for a in train_dock.build_arg_parser()._actions):
        return ["--learning-rate", lr]
    d = json.loads(json.dumps(dock))
    d.setdefault("algorithms", {}).setdefault("ppo", {})["learning_rate"] = float(lr)
    path = tmp_path / f"dock_lr_{lr}.yaml"
    path.write_text(yaml.safe_dump(d))
    return ["--config", str(path)]
