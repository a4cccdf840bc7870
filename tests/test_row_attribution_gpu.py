"""Row attribution of kp1_mlp_loss_grad and kp1_mlp_anchor_loss_grad at n = 2065: every row of the minibatch contributes exactly nothing
except 24 spike rows placed where the kernels change tile, stage or chunk (tests/row_attribution.py derives the places from the launch
code), so the gradient must equal the fp64 autograd gradient of those 24 rows alone -- under the project's unchanged tolerance, per tensor
2e-4 * max|ref| + 1e-7.  A row dropped, counted twice or credited to another chunk or replica is then an error of several percent of a
tensor's scale, where the full-minibatch tests at this n see 1e-4 of it.  test_row_attribution_cpu.py asserts the conditions behind that
(spikes inside the clip range, silent rows silent in fp64, every spike worth >= 10 tolerances, the positions cover the launch's boundaries)."""
from __future__ import annotations

import pytest
import torch

import mlp_handle_state as S
import row_attribution as R
from rl_brain_trainer_amd.mlp import MlpKernels

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAN = float("nan")
POP = [((h, d, "layer"), True, 3) for h, d in S.POP_KINDS]
LOSS_CASES = [(kd, gather, 1) for kd in S.KINDS for gather in (True, False)] + POP
ANCHOR_CASES = [(kd, gather, 1) for kd in R.ANCHOR_KINDS for gather in (True, False)] + POP


def _ids(cases):
    return [f"{kd[0]}-{kd[1]}-{kd[2]}-K{K}-{'idx' if gather else 'prefix'}" for kd, gather, K in cases]


@pytest.fixture(scope="module")
def world():
    """per (hidden, obs_dim, gather, K): the CPU case (shared by the fused and the layer-wise 2x256 handle) and its device copies"""
    cache = {}

    def get(kind, gather, K):
        key = (kind[0], kind[1], gather, K)
        if key not in cache:
            c = R.build(kind[0], kind[1], gather=gather, K=K)
            cache[key] = (c, {name: c[name].to(DEV).contiguous() for name in ("obs", "act", "old_logp", "flat", "idx")})
        return cache[key]

    return get


def _handle(kind, K) -> MlpKernels:
    hidden, obs_dim, path = kind
    k = MlpKernels(hidden, DEV, max_batch=R.MAX_BATCH, obs_dim=obs_dim, replicas=K)
    if hidden == 256:
        k.set_fused(path == "fused")
    return k


def _own_outputs(k: MlpKernels, d: dict, K: int):
    """the handle's own deterministic mean [K][n][7] and value [K][n] of the minibatch rows, by batch position"""
    rows = d["obs"][d["idx"].reshape(-1)].contiguous()
    mean, value = torch.full((K * R.N, 7), NAN, device=DEV), torch.full((K * R.N,), NAN, device=DEV)
    k.forward(rows, mean=mean, value=value)
    return mean.view(K, R.N, 7), value.view(K, R.N)


def _compare(grad, ref_grad, spec, side, what) -> float:
    """active tensors within the tolerance, the others exactly zero; returns the worst error / tolerance"""
    on = R.active(side)
    errs = R.grad_errors(grad, ref_grad, spec)
    for name, sl in S.slices_of(spec).items():
        if not on(name):
            assert torch.equal(grad[sl], torch.zeros_like(grad[sl])), (what, name, "must be exactly 0")
    bad = {name: round(e, 3) for name, e in errs.items() if on(name) and not e <= 1.0}
    assert not bad, (what, "error / tolerance", bad)
    return max(e for name, e in errs.items() if on(name))


@pytest.mark.parametrize("kind,gather,K", LOSS_CASES, ids=_ids(LOSS_CASES))
def test_loss_grad_equals_the_gradient_of_its_spike_rows(world, kind, gather, K):
    """Raw advantages, ent_coef = 0, inv_count = 1 / 24.  Policy side: vf_coef = 0 and advantage 0 on the silent rows (g_logp = -0 * ratio *
    inv_count, so every partial of a silent row is exactly 0 and the value net's gradient is exactly 0).  Value side: advantage 0 everywhere,
    vf_coef = 0.5, the return of a silent row = the value this handle's forward computes for it (the training path may differ from that by ulps:
    about 1e-7 per row, random in sign, against spikes of [1, 2]).  K = 3: each replica its own rows, policy and spike values."""
    c, d = world(kind, gather, K)
    spec, Pn = c["spec"], c["flat"].shape[1]
    k = _handle(kind, K)
    k.pack(d["flat"])
    idx = d["idx"].contiguous() if (gather or K > 1) else None
    _, own_value = _own_outputs(k, d, K)
    for side, vf in (("policy", 0.0), ("value", R.VF_COEF)):
        buf = R.policy_side(c) if side == "policy" else R.value_side(c, own_value)
        adv, ret = buf["adv"].to(DEV), buf["ret"].to(DEV)
        grad, stats = torch.full((K, Pn), NAN, device=DEV), torch.zeros((K, 4), device=DEV)
        k.loss_grad(d["obs"], idx, R.N, d["act"], d["old_logp"], adv, ret, clip_range=R.CLIP_RANGE, ent_coef=0.0, vf_coef=vf, inv_count=1.0 / R.NS,
                    grad_out=grad, stats_out=stats, normalize=False)
        grad = grad.cpu()
        assert torch.isfinite(grad).all() and torch.isfinite(stats).all()
        for r in range(K):
            ref = R.loss_reference(c, buf, r, c["spike_rows"][r], vf)
            worst = _compare(grad[r], ref["grad"], spec, side, (kind, gather, side, r))
            print(f"{kind} {'idx' if gather else 'prefix'} K={K} replica {r} {side} side: worst gradient error / tolerance {worst:.3f}")
    k.close()


@pytest.mark.parametrize("kind,gather,K", ANCHOR_CASES, ids=_ids(ANCHOR_CASES))
def test_anchor_loss_grad_equals_the_gradient_of_its_spike_rows(world, kind, gather, K):
    """kp1_mlp_anchor_loss_grad on the same minibatches: teacher action of a silent row = this handle's own deterministic mean, of a spike the
    mean + sign x [0.5, 1] per component.  The kernel's mean runs over all n rows, so the reference is the sum over S / (7 n).  The gradient
    of every tensor outside the six actor tensors is exactly 0 (include/kp1_ppo.h); the loss within the anchor tests' 2e-4 relative."""
    c, d = world(kind, gather, K)
    spec, Pn = c["spec"], c["flat"].shape[1]
    k = _handle(kind, K)
    k.pack(d["flat"])
    idx = d["idx"].contiguous() if (gather or K > 1) else None
    own_mean, _ = _own_outputs(k, d, K)
    teacher = R.anchor_side(c, own_mean)
    grad, loss = torch.full((K, Pn), NAN, device=DEV), torch.full((K,), NAN, device=DEV)
    k.anchor_loss_grad(d["obs"], idx, R.N, teacher.to(DEV), loss_weight=R.LOSS_WEIGHT, grad_out=grad, loss_out=loss)
    grad, loss = grad.cpu(), loss.cpu()
    assert torch.isfinite(grad).all()
    for r in range(K):
        ref = R.anchor_reference(c, teacher, r, c["spike_rows"][r])
        worst = _compare(grad[r], ref["grad"], spec, "anchor", (kind, gather, "anchor", r))
        rel = abs(loss[r].item() - ref["loss"]) / ref["loss"]
        print(f"{kind} {'idx' if gather else 'prefix'} K={K} replica {r} anchor: worst gradient error / tolerance {worst:.3f}, loss relative error {rel:.2e}")
        assert rel <= 2e-4, (kind, gather, r, loss[r].item(), ref["loss"])
    k.close()
