"""The teacher-anchor side loss as a device step (kp1_mlp_anchor_loss_grad / kp1_mlp_anchor_adam_step, PopulationTeacherAnchor,
``train_route --seeds`` with ``route.teacher_anchor.enabled``): gradients against torch autograd, the step against an fp64 restatement of
``RouteTeacherAnchor.gradient_step`` with a bound measured from the shipped torch step, what the step must leave untouched, population =
single handles, population trainer = K = 1 trainers and graphs = eager, the CLI, and the refusals."""
from __future__ import annotations

import ctypes as C
import json
import math

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import mlp as M
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import ppo as P
from rl_brain_trainer_amd import route_config as rcfg
from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv, RouteVecEnv
from rl_brain_trainer_amd.teacher_anchor import ACTOR_TENSORS, PopulationTeacherAnchor, RouteTeacherAnchor, TeacherAnchorConfig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
IN, W = 80, 128


def _cfg() -> dict:
    return json.loads((GOLDEN / "configs" / "route_curriculum_prefix120_routeobs_sequence2.json").read_text())


def _route_q():
    return rcfg.load_route_q(GOLDEN / "synthetic_route.json")


def _offsets(spec) -> dict[str, tuple[int, tuple[int, ...]]]:
    out, o = {}, 0
    for name, shape in spec:
        out[name] = (o, shape)
        o += math.prod(shape)
    return out


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """observations of the device env under a servo toward the route goal, teacher = clip(0.8 * route_q_error): 16 envs x 64 steps; the
    protected prefix (max_route_index) is the 60 % quantile of the recorded waypoint indices, so the filter drops rows"""
    cfgd = _cfg()
    env = RouteVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=30), _route_q(), 16, seed=3)
    rows, acts, ridx = [], [], []
    obs = env.reset()
    for _ in range(64):
        a = (0.8 * RouteVecEnv.obs_dict(obs)["route_q_error"]).clamp(-1, 1)
        rows.append(obs[:, :IN].cpu().numpy().copy())
        acts.append(a.cpu().numpy().copy())
        ridx.append(env.info()["route_index"].cpu().numpy().copy())
        obs, _, _ = env.step(a)
    env.close()
    rows, acts, ridx = np.concatenate(rows).astype(np.float32), np.concatenate(acts).astype(np.float32), np.concatenate(ridx).astype(np.int32)
    path = tmp_path_factory.mktemp("anchor") / "teacher.npz"
    np.savez(path, actions=acts, route_index=ridx, **{f"obs__{k}": rows[:, o:o + w] for k, (o, w) in rcfg.ROUTE_OBS_LAYOUT.items()})
    prefix = int(np.quantile(ridx, 0.6))
    keep = ridx <= prefix
    assert 256 < int(keep.sum()) < len(ridx), (prefix, int(keep.sum()))        # the prefix filter drops rows and more than one batch is left
    obs_pad = torch.zeros((int(keep.sum()), W), device=DEV)
    obs_pad[:, :IN] = torch.as_tensor(rows[keep], device=DEV)
    return {"path": str(path), "max_route_index": prefix, "obs": obs_pad, "actions": torch.as_tensor(acts[keep], device=DEV).contiguous(), "rows": int(keep.sum())}


@pytest.fixture(scope="module", params=[64, 128])
def world(request, dataset):
    """a single route PPO of the given width after one update (non-trivial Adam state, adam_t > 0), with a snapshot to restore"""
    cfgd = _cfg()
    env = RouteVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=40), _route_q(), 16, seed=11)
    pc = P.PPOConfig(n_steps=64, batch_size=256, n_epochs=2, hidden=request.param, learning_rate=3e-4, ent_coef=1e-3, seed=5)
    ppo = P.PPO(env, pc, use_graphs=False)
    ppo.collect_rollouts()
    ppo.train()
    assert ppo.adam_t > 0 and ppo._mlp.replicas == 1
    snap = (ppo.policy.flat.clone(), ppo.adam_m.clone(), ppo.adam_v.clone())

    def restore() -> None:
        ppo.policy.flat.copy_(snap[0])
        ppo.adam_m.copy_(snap[1])
        ppo.adam_v.copy_(snap[2])
        ppo.actor_extra_steps = 0
        ppo._mlp.pack(ppo.policy.flat)
        ppo._mlp.set_step_count(ppo.adam_t)
        ppo._mlp.set_actor_extra_steps(0)

    yield {"ppo": ppo, "restore": restore, "hidden": request.param, "off": _offsets(ppo.policy.spec)}
    env.close()


def _batch(dataset, n: int, seed: int = 0) -> torch.Tensor:
    return torch.as_tensor(np.random.default_rng(seed).integers(0, dataset["rows"], size=n), device=DEV)


# ---------------------------------------------------------------------------------------------------------------- 1. gradients
@pytest.mark.parametrize("n", [256, 40])
def test_anchor_gradient_matches_autograd(world, dataset, n):
    """K = 1 handle; n = 40 is a tail tile (what M < batch_size produces).  Per tensor 2e-4 * max|ref| + 1e-7 (the project's fp32
    summation-order tolerance, tests/test_route_ppo_gpu.py), loss 2e-4 relative, every non-actor element exactly 0."""
    ppo = world["ppo"]
    world["restore"]()
    mlp = ppo._mlp
    idx = _batch(dataset, n, seed=n)
    grad = torch.full((mlp.num_params,), 7.0, device=DEV)
    loss = torch.full((1,), -1.0, device=DEV)
    mlp.anchor_loss_grad(dataset["obs"], idx, n, dataset["actions"], loss_weight=0.5, grad_out=grad, loss_out=loss)
    views = ppo.policy.views
    leaves = {name: views[name].detach().clone().requires_grad_(True) for name in ACTOR_TENSORS}
    mean, _ = P.mlp_forward({**views, **leaves}, dataset["obs"][idx, :IN])
    ref_loss = torch.nn.functional.mse_loss(mean, dataset["actions"][idx]) * 0.5
    ref = dict(zip(ACTOR_TENSORS, torch.autograd.grad(ref_loss, [leaves[k] for k in ACTOR_TENSORS])))
    for name, (o, shape) in world["off"].items():
        got = grad[o:o + math.prod(shape)].view(shape)
        if name in ref:
            scale = ref[name].abs().max().item()
            err = (got - ref[name]).abs().max().item()
            print(f"hidden={world['hidden']} n={n} {name}: err {err:.3e} max|ref| {scale:.3e}")
            assert scale > 0 and err <= 2e-4 * scale + 1e-7, name
        else:
            assert torch.all(got == 0), name
    print(f"loss {loss.item():.8e} ref {ref_loss.item():.8e}")
    assert abs(loss.item() - ref_loss.item()) <= 2e-4 * abs(ref_loss.item())


# ---------------------------------------------------------------------------------------------------------------- 2. step
def _restate_fp64(ppo, obs: torch.Tensor, teacher: torch.Tensor, *, loss_weight: float, step: int) -> dict:
    """RouteTeacherAnchor.gradient_step in fp64 on the CPU, from the fp32 state of `ppo`"""
    cfg = ppo.cfg
    flat, m, v = ppo.policy.flat.double().cpu(), ppo.adam_m.double().cpu(), ppo.adam_v.double().cpu()
    off = _offsets(ppo.policy.spec)
    views = {name: flat[o:o + math.prod(shape)].view(shape) for name, (o, shape) in off.items()}
    leaves = {name: views[name].clone().requires_grad_(True) for name in ACTOR_TENSORS}
    mean, _ = P.mlp_forward({**views, **leaves}, obs.double().cpu())
    loss = torch.nn.functional.mse_loss(mean, teacher.double().cpu()) * loss_weight
    grads = torch.autograd.grad(loss, [leaves[k] for k in ACTOR_TENSORS])
    norm = math.sqrt(sum(float((g * g).sum()) for g in grads))
    scale = min(0.5 / (norm + 1e-6), 1.0)
    bc1, bc2 = 1.0 - 0.9 ** step, 1.0 - 0.999 ** step
    out = {"norm": norm, "loss": float(loss.detach()), "params": {}, "exp_avg": {}}
    for name, g in zip(ACTOR_TENSORS, grads):
        o, shape = off[name]
        sl = slice(o, o + math.prod(shape))
        g = (g * scale).reshape(-1)
        mn = 0.9 * m[sl] + 0.1 * g
        vn = 0.999 * v[sl] + 0.001 * g * g
        out["exp_avg"][name] = mn
        out["params"][name] = flat[sl] - (cfg.learning_rate / bc1) * mn / (vn.sqrt() / math.sqrt(bc2) + cfg.adam_eps)
    return out


@pytest.mark.parametrize("case", ["clipped", "unclipped"])
def test_anchor_step_against_fp64_restatement(world, dataset, case):
    """After one PPO update.  Per actor tensor, for the parameters and exp_avg:
        |device step - fp64 restatement| <= 8 * max(|RouteTeacherAnchor.gradient_step - fp64 restatement|, one fp32 ulp of max|tensor|)
    (both are fp32 evaluations that differ in summation order over three chained GEMMs and a norm).  loss_weight is chosen from the fp64
    restatement at weight 1 so that its gradient norm is 2.0 (clipped at 0.5) or 0.125 (not clipped); asserted on the restatement.
    Values of one MI355X run: profiles/r11_anchor_parity.json."""
    ppo, restore = world["ppo"], world["restore"]
    restore()
    n = 256
    idx = _batch(dataset, n)
    obs_b, act_b = dataset["obs"][idx, :IN].contiguous(), dataset["actions"][idx].contiguous()
    step = ppo.adam_t + 1
    unit = _restate_fp64(ppo, obs_b, act_b, loss_weight=1.0, step=step)["norm"]
    weight = (2.0 if case == "clipped" else 0.125) / unit
    ref = _restate_fp64(ppo, obs_b, act_b, loss_weight=weight, step=step)
    assert ref["norm"] > 1.0 if case == "clipped" else ref["norm"] < 0.25, ref["norm"]

    anchor = RouteTeacherAnchor(TeacherAnchorConfig(enabled=True, dataset_path=dataset["path"], loss_weight=weight, batch_size=n,
                                                    max_route_index=dataset["max_route_index"]))
    torch_loss = anchor.gradient_step(ppo, obs_b, act_b)
    torch_p, torch_m = ppo.policy.flat.clone(), ppo.adam_m.clone()
    restore()
    mlp = ppo._mlp
    grad = torch.empty(mlp.num_params, device=DEV)
    loss = torch.empty(1, device=DEV)
    mlp.anchor_loss_grad(dataset["obs"], idx, n, dataset["actions"], loss_weight=weight, grad_out=grad, loss_out=loss)
    mlp.anchor_adam_step(ppo.policy.flat, grad, ppo.adam_m, ppo.adam_v, lr=ppo.cfg.learning_rate, eps=ppo.cfg.adam_eps, max_grad_norm=0.5, step=ppo.adam_t)
    dev_p, dev_m = ppo.policy.flat.clone(), ppo.adam_m.clone()
    restore()
    print(f"hidden={world['hidden']} {case}: fp64 norm {ref['norm']:.6f} loss fp64 {ref['loss']:.8e} torch {torch_loss:.8e} device {loss.item():.8e}")
    failures = []
    for what, dev, tor in (("params", dev_p, torch_p), ("exp_avg", dev_m, torch_m)):
        for name in ACTOR_TENSORS:
            o, shape = world["off"][name]
            sl = slice(o, o + math.prod(shape))
            r = ref[what][name]
            e_dev = (dev[sl].double().cpu() - r).abs().max().item()
            e_torch = (tor[sl].double().cpu() - r).abs().max().item()
            ulp = float(np.spacing(np.float32(r.abs().max().item())))
            bound = 8.0 * max(e_torch, ulp)
            print(f"  {what:8s} {name:36s} device {e_dev:.3e} torch {e_torch:.3e} ulp {ulp:.3e} bound {bound:.3e}")
            if not e_dev <= bound:
                failures.append((what, name, e_dev, bound))
            if what == "params":
                assert (dev[sl] != ppo.policy.flat[sl]).any(), name      # the step moved the tensor (ppo holds the restored snapshot)
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------- 3. untouched state
def _probe(ppo) -> torch.Tensor:
    """the parameters one kp1_mlp_adam_step(step = 0) produces from fixed scratch tensors: a function of the device-resident step count and
    of the actor-extra count (both enter the bias corrections).  The handle's packed weights are restored afterwards."""
    mlp = ppo._mlp
    g = torch.Generator(device="cpu").manual_seed(3)
    n = mlp.num_params
    p, grad = torch.randn(n, generator=g).to(DEV), (1e-3 * torch.randn(n, generator=g)).to(DEV)
    m, v = (1e-3 * torch.randn(n, generator=g)).to(DEV), (1e-6 * torch.rand(n, generator=g)).to(DEV)
    mlp.adam_step(p, grad, m, v, lr=3e-4, eps=1e-5, max_grad_norm=0.5, step=0, fused_norm=False)
    mlp.pack(ppo.policy.flat)
    return p


def test_anchor_step_leaves_the_rest_untouched(world, dataset):
    ppo, restore, off = world["ppo"], world["restore"], world["off"]
    restore()
    mlp = ppo._mlp
    n = 200
    idx = _batch(dataset, n, seed=5)
    rest = [name for name, _ in ppo.policy.spec if name not in ACTOR_TENSORS]
    assert "log_std" in rest and "value_net.weight" in rest and len(rest) == 7

    def run():
        restore()
        grad, loss = torch.empty(mlp.num_params, device=DEV), torch.empty(1, device=DEV)
        mlp.anchor_loss_grad(dataset["obs"], idx, n, dataset["actions"], loss_weight=0.5, grad_out=grad, loss_out=loss)
        mlp.anchor_adam_step(ppo.policy.flat, grad, ppo.adam_m, ppo.adam_v, lr=3e-4, eps=1e-5, max_grad_norm=0.5, step=ppo.adam_t)
        return [t.clone() for t in (ppo.policy.flat, ppo.adam_m, ppo.adam_v, grad, loss)]

    restore()
    before = [t.clone() for t in (ppo.policy.flat, ppo.adam_m, ppo.adam_v)]
    c0 = _probe(ppo)
    grad, loss = torch.empty(mlp.num_params, device=DEV), torch.empty(1, device=DEV)
    mlp.anchor_loss_grad(dataset["obs"], idx, n, dataset["actions"], loss_weight=0.5, grad_out=grad, loss_out=loss)
    assert torch.equal(_probe(ppo), c0)                      # neither the step count nor the actor-extra count moved
    mlp.set_step_count(ppo.adam_t + 1)
    assert not torch.equal(_probe(ppo), c0)                  # (the probe does see a moved step count)
    mlp.set_step_count(ppo.adam_t)
    mlp.anchor_adam_step(ppo.policy.flat, grad, ppo.adam_m, ppo.adam_v, lr=3e-4, eps=1e-5, max_grad_norm=0.5, step=ppo.adam_t)
    # the packed weights follow: the handle's forward equals a fresh handle packed from the flat vector, and torch on the views
    rows = dataset["obs"][:96].contiguous()
    mean = torch.empty((96, 7), device=DEV)
    mlp.forward(rows, mean=mean)
    fresh = M.MlpKernels(world["hidden"], DEV, max_batch=128, obs_dim=IN)
    fresh.pack(ppo.policy.flat)
    mean_fresh = torch.empty_like(mean)
    fresh.forward(rows, mean=mean_fresh)
    fresh.close()
    assert torch.equal(mean, mean_fresh)
    ref_mean, _ = P.mlp_forward(ppo.policy.views, rows[:, :IN])
    assert torch.allclose(mean, ref_mean, rtol=1e-4, atol=2e-5)
    after = [t.clone() for t in (ppo.policy.flat, ppo.adam_m, ppo.adam_v)]
    for name, (o, shape) in off.items():
        sl = slice(o, o + math.prod(shape))
        for what, b, a in zip(("params", "exp_avg", "exp_avg_sq"), before, after):
            if name in rest:
                assert torch.equal(b[sl], a[sl]), (what, name)
            else:
                assert (b[sl] != a[sl]).any(), (what, name)
    # actor_extra is one larger: the probe equals the probe at an explicitly set count of 1, and differs from the count-0 probe
    c1 = _probe(ppo)
    mlp.set_actor_extra_steps(1)
    assert torch.equal(_probe(ppo), c1) and not torch.equal(c1, c0)
    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert torch.equal(first[0], after[0]) and torch.equal(first[1], after[1]) and torch.equal(first[2], after[2])
    restore()


# ---------------------------------------------------------------------------------------------------------------- 4. population = single
@pytest.mark.parametrize("hidden", [64, 128])
def test_anchor_population_equals_single_handles(dataset, hidden):
    K, n = 3, 200
    g = torch.Generator(device="cpu").manual_seed(hidden)
    pols = [P.ActorCritic(hidden, DEV, seed=21 + k, obs_dim=IN) for k in range(K)]
    for p in pols:
        p.flat.add_(0.05 * torch.randn(p.numel, generator=g).to(DEV))
    NP = pols[0].numel
    flat = torch.stack([p.flat for p in pols]).contiguous()
    m0, v0 = (1e-3 * torch.randn((K, NP), generator=g)).to(DEV), (1e-6 * torch.rand((K, NP), generator=g)).to(DEV)
    hp = [dict(learning_rate=lr, adam_eps=eps, max_grad_norm=0.3 + k, clip_range=0.2, ent_coef=1e-3, vf_coef=0.5)
          for k, (lr, eps) in enumerate([(3e-4, 1e-5), (1e-4, 1e-7), (1e-3, 1e-6)])]
    idx = torch.stack([_batch(dataset, n, seed=10 + k) for k in range(K)]).contiguous()
    pop = M.MlpKernels(hidden, DEV, max_batch=n, obs_dim=IN, replicas=K)
    pop.pack(flat)
    pop.set_replica_hparams(hp)
    pop.set_step_count(5)
    pop.set_actor_extra_steps(2)
    params, m, v = flat.clone(), m0.clone(), v0.clone()
    grad, loss = torch.empty((K, NP), device=DEV), torch.empty(K, device=DEV)
    for step in (0, 9):          # the device-resident count, then a count given by the caller
        pop.anchor_loss_grad(dataset["obs"], idx, n, dataset["actions"], loss_weight=2.0, grad_out=grad, loss_out=loss)
        pop.anchor_adam_step(params, grad, m, v, lr=7.0, eps=7.0, max_grad_norm=0.5, step=step)      # lr / eps come from the table
    for k in range(K):
        one = M.MlpKernels(hidden, DEV, max_batch=n, obs_dim=IN)
        one.pack(flat[k].contiguous())
        one.set_step_count(5)
        one.set_actor_extra_steps(2)
        pk, mk, vk = flat[k].clone(), m0[k].clone(), v0[k].clone()
        gk, lk = torch.empty(NP, device=DEV), torch.empty(1, device=DEV)
        for step in (0, 9):
            one.anchor_loss_grad(dataset["obs"], idx[k].contiguous(), n, dataset["actions"], loss_weight=2.0, grad_out=gk, loss_out=lk)
            one.anchor_adam_step(pk, gk, mk, vk, lr=hp[k]["learning_rate"], eps=hp[k]["adam_eps"], max_grad_norm=0.5, step=step)
        for name, a, b in (("params", pk, params[k]), ("exp_avg", mk, m[k]), ("exp_avg_sq", vk, v[k]), ("grad", gk, grad[k]), ("loss", lk[0], loss[k])):
            assert torch.equal(a, b), (name, k)
        assert not torch.equal(pk, flat[k])
        one.close()
    assert not torch.equal(loss[0], loss[1])
    pop.close()


# ---------------------------------------------------------------------------------------------------------------- 5. trainer
_TRAINED: dict = {}


def _train(dataset, seeds: tuple[int, ...], use_graphs: bool) -> dict:
    """three iterations (n_steps 64, minibatch 256) of RoutePopulationPPO(seeds) with an anchor of its own (every 2nd rollout, 2 gradient
    steps); cached per argument"""
    key = (seeds, use_graphs)
    if key in _TRAINED:
        return _TRAINED[key]
    from rl_brain_trainer_amd.population import RoutePopulationPPO

    cfgd = _cfg()
    env = RoutePopulationVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=10), _route_q(), list(seeds), 16)
    anchor = PopulationTeacherAnchor(TeacherAnchorConfig(enabled=True, dataset_path=dataset["path"], loss_weight=0.5, batch_size=256, gradient_steps=2,
                                                         every_rollouts=2, max_route_index=dataset["max_route_index"]))
    pcfg = P.PPOConfig(n_steps=64, batch_size=256, n_epochs=2, hidden=64, learning_rate=2e-4, ent_coef=1e-3)
    pop = RoutePopulationPPO(list(seeds), pcfg, env, use_graphs=use_graphs, teacher_anchor=anchor)
    losses = []
    for it in range(3):
        # The route env has no device snapshot, so a rollout graph captured before any eager rollout starts its episodes from one extra
        # reset() draw (PPO._capture_rollout).  A step callback makes the first rollout eager in every run: the runs then differ only in
        # what is under test -- the update graph is captured in the first train(), before the first anchor step, and the rollout graph at
        # the second rollout.
        pop.step_callback = (lambda done: None) if it == 0 else None
        pop.collect_rollouts()
        anchor.on_rollout_end(pop)
        losses.append(list(anchor.last_loss))
        pop.train()
    torch.cuda.synchronize()
    out = {"flat": pop.flat.clone(), "m": pop.adam_m.clone(), "v": pop.adam_v.clone(), "losses": losses, "extra": pop.actor_extra_steps,
           "view_extra": pop.replica(0).actor_extra_steps, "adam_t": pop.adam_t}
    pop.close()
    env.close()
    _TRAINED[key] = out
    return out


def test_anchor_population_trainer_equals_single_trainers(dataset):
    both = _train(dataset, (7, 8), False)
    assert both["extra"] == both["view_extra"] == 2 and both["adam_t"] == 3 * 2 * 4        # one anchored rollout of two steps in three
    assert both["losses"][0] == [0.0, 0.0] and all(v > 0 for v in both["losses"][1]) and both["losses"][2] == both["losses"][1]
    for k, s in enumerate((7, 8)):
        one = _train(dataset, (s,), False)
        for name in ("flat", "m", "v"):
            assert torch.equal(one[name][0], both[name][k]), (name, s)
        assert [l[0] for l in one["losses"]] == [l[k] for l in both["losses"]], s      # the shared index stream
        assert one["extra"] == 2
    assert not torch.equal(both["flat"][0], both["flat"][1])


def test_anchor_population_trainer_graphs_equal_eager(dataset):
    """the update graph captured before the first anchor step reads the new actor count when it is replayed"""
    eager, graphs = _train(dataset, (7, 8), False), _train(dataset, (7, 8), True)
    for name in ("flat", "m", "v"):
        assert torch.equal(eager[name], graphs[name]), name
    assert eager["losses"] == graphs["losses"] and graphs["extra"] == 2


# ---------------------------------------------------------------------------------------------------------------- 6. CLI
def test_train_route_cli_seeds_with_teacher_anchor(tmp_path, dataset):
    from rl_brain_trainer_amd import checkpoint as ck
    from rl_brain_trainer_amd import train_route

    cfgd = _cfg()
    cfgd["route"]["curriculum"] = {**cfgd["route"].get("curriculum", {}), "prefix_stages": [10, 20], "promotion_window_episodes": 16,
                                   "min_episodes_per_stage": 16, "promotion_success_rate": 0.0, "promotion_route_ready_hit_rate": 0.0,
                                   "promotion_orientation_hit_rate": 0.0, "promotion_max_regression_rate": 1.0}
    cfgd["route"]["teacher_anchor"] = {"enabled": True, "dataset_path": dataset["path"], "loss_weight": 0.02, "batch_size": 128, "gradient_steps": 2,
                                       "max_route_index": dataset["max_route_index"]}
    cfgd["route"]["sequential_gate"] = {"enabled": False}
    cfgd["route"]["route_path"] = str(GOLDEN / "synthetic_route.json")
    cfgd["route"].pop("init_checkpoint", None)
    cfg_path = tmp_path / "route.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgd))
    out = tmp_path / "pop"
    summary = train_route.main(["--config", str(cfg_path), "--n-envs", "16", "--n-steps", "64", "--batch-size", "256", "--hidden", "64", "--run-id", "pop",
                                "--output-dir", str(out), "--total-timesteps", "2048", "--seeds", "7,8", "--log-every", "1"])
    steps = 2 * 2                                   # two rollouts, two gradient steps after each
    assert summary["teacher_anchor_steps"] == steps
    assert json.loads((out / "population_summary.json").read_text())["teacher_anchor_steps"] == steps
    spec = P.param_spec(64, IN)
    for s in (7, 8):
        ts = json.loads((out / f"seed_{s}" / "training_summary.json").read_text())
        assert ts["teacher_anchor_summary"]["enabled"] is True and ts["teacher_anchor_summary"]["sample_count"] == dataset["rows"] > 0
        opt = ck.load_optimizer_state_dict(out / f"seed_{s}" / "model_latest.zip")
        actor = {float(opt["state"][i]["step"]) for i, (name, _) in enumerate(spec) if name in ACTOR_TENSORS}
        rest = {float(opt["state"][i]["step"]) for i, (name, _) in enumerate(spec) if name not in ACTOR_TENSORS}
        assert len(actor) == len(rest) == 1 and actor.pop() - rest.pop() == steps, s


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_anchor_entry_points_refuse_before_any_launch(dataset):
    one = M.MlpKernels(64, DEV, max_batch=256, obs_dim=IN)
    L, vp = one.L, C.c_void_p
    NP = one.num_params
    grad, loss = torch.full((3 * NP,), 5.0, device=DEV), torch.full((3,), 5.0, device=DEV)
    scratch = torch.zeros(3 * NP, device=DEV)
    obs, act = dataset["obs"], dataset["actions"]
    p = lambda t: vp(t.data_ptr())      # noqa: E731
    stream = vp(torch.cuda.current_stream(DEV).cuda_stream)

    def refused(rc: int, code: int, text: str) -> None:
        assert rc == code and text in L.kp1_last_error().decode(), (rc, L.kp1_last_error())

    INVALID, UNSUPPORTED = -1, -4
    for hole in range(5):           # NULL handle, obs, teacher, grad_out, loss_out
        args = [one._h, p(obs), W, None, 64, p(act), 0.5, p(grad), p(loss), stream]
        args[{0: 0, 1: 1, 2: 5, 3: 7, 4: 8}[hole]] = None
        refused(L.kp1_mlp_anchor_loss_grad(*args), INVALID, "NULL")
    for n in (0, -3, one.max_batch + 1):
        refused(L.kp1_mlp_anchor_loss_grad(one._h, p(obs), W, None, n, p(act), 0.5, p(grad), p(loss), stream), INVALID, "max_batch")
    for stride in (0, 56, 64, 100):
        refused(L.kp1_mlp_anchor_loss_grad(one._h, p(obs), stride, None, 64, p(act), 0.5, p(grad), p(loss), stream), INVALID, "obs_stride")
    for hole in range(5):           # NULL handle, params, grad, exp_avg, exp_avg_sq
        args = [one._h, p(scratch), p(grad), p(scratch), p(scratch), 3e-4, 1e-5, 0.5, 1, stream]
        args[hole] = None
        refused(L.kp1_mlp_anchor_adam_step(*args), INVALID, "NULL")
    wide = M.MlpKernels(256, DEV, max_batch=256, obs_dim=IN)
    refused(L.kp1_mlp_anchor_loss_grad(wide._h, p(obs), W, None, 64, p(act), 0.5, p(grad), p(loss), stream), UNSUPPORTED, "hidden must be 64 or 128")
    refused(L.kp1_mlp_anchor_adam_step(wide._h, p(scratch), p(grad), p(scratch), p(scratch), 3e-4, 1e-5, 0.5, 1, stream), UNSUPPORTED, "hidden must be 64 or 128")
    with pytest.raises(native.Kp1Error, match="hidden must be 64 or 128"):
        wide.anchor_loss_grad(obs, None, 64, act, loss_weight=0.5, grad_out=torch.zeros(wide.num_params, device=DEV), loss_out=loss[:1])
    wide.close()
    pop = M.MlpKernels(64, DEV, max_batch=256, obs_dim=IN, replicas=3)
    refused(L.kp1_mlp_anchor_loss_grad(pop._h, p(obs), W, None, 64, p(act), 0.5, p(grad), p(loss), stream), INVALID, "idx")
    pop.close()
    torch.cuda.synchronize()
    assert torch.all(grad == 5.0) and torch.all(loss == 5.0) and torch.all(scratch == 0)      # nothing was launched
    one.close()
