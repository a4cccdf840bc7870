"""Shared by test_mlp_handle_state_gpu.py and test_mlp_handle_state_cpu.py: policies, sample buffers and the fp64 references of the
training-handle tests.  The inputs and references are plain torch on the CPU (the GPU module moves the inputs over), so the conditions that
give the GPU checks their power can be asserted without a GPU on exactly the inputs the GPU tests use.  The call helpers of the GPU
modules (handle, dev, loss_grad, check_kl) live here too, shared with test_trained_regime_gpu.py."""
from __future__ import annotations

import math

import numpy as np
import torch

from rl_brain_trainer_amd import ppo as P

CPU = torch.device("cpu")
# (hidden, obs_dim, path): the five handle kinds; the population kinds are (hidden, obs_dim) with K = 3 on the layer-wise kernels
KINDS = [(256, 56, "fused"), (256, 80, "fused"), (256, 56, "layer"), (128, 80, "layer"), (64, 56, "layer")]
POP_KINDS = [(64, 56), (128, 80)]
KIND_IDS = [f"{h}-{d}-{p}" for h, d, p in KINDS]
TOTAL = 512
LOG_STD = (-0.3, 0.1, -0.5, 0.0, 0.2, -0.1, -0.7)


def pitch(obs_dim: int) -> int:
    return 64 if obs_dim <= 64 else 128


def policy(hidden: int, obs_dim: int, device=CPU, seed: int = 3, head_scale: float = 1.0) -> P.ActorCritic:
    """test_ppo_kernels_gpu._policy: orthogonal weights, non-zero biases and log_std (all drawn on the CPU, so the same on every device)"""
    pol = P.ActorCritic(hidden, device, seed=seed, obs_dim=obs_dim)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    for name, _ in pol.spec:
        if name.endswith("bias"):
            pol.views[name].copy_(0.1 * torch.randn(pol.views[name].shape, generator=g))
    pol.views["log_std"].copy_(torch.tensor(LOG_STD))
    if head_scale != 1.0:
        pol.views["action_net.weight"].mul_(head_scale)
    return pol


def views_of(flat: torch.Tensor, spec) -> dict[str, torch.Tensor]:
    out, off = {}, 0
    for name, shape in spec:
        cnt = math.prod(shape)
        out[name] = flat[off:off + cnt].view(shape)
        off += cnt
    return out


def slices_of(spec) -> dict[str, slice]:
    out, off = {}, 0
    for name, shape in spec:
        cnt = math.prod(shape)
        out[name] = slice(off, off + cnt)
        off += cnt
    return out


def sample_buffers(flat: torch.Tensor, spec, obs_dim: int, *, total: int = TOTAL, seed: int = 1, adv_scale: float = 3.0, adv_shift: float = 0.5,
                   ret_shift: float = 0.0, obs_scale: float = 1.0, old_shift_rel: bool = False, clip_share: float = 0.0) -> dict[str, torch.Tensor]:
    """test_mlp_loss_grad_vs_torch_autograd's sample buffers on the CPU: observations at the padded pitch (pad columns zero), actions sampled
    from the policy, old log-probs from a slightly different policy so that ratios spread around 1 and both clip branches occur.
    old_shift_rel: the old policy's mean is shifted by 0.05 sigma randn in place of 0.05 randn (at a trained sigma of 0.02 .. 0.1 the
    absolute shift is many sigma and every ratio leaves the clip range).  clip_share: that share of the real observation entries, chosen by
    a generator of its own, is replaced by its sign before obs_scale is applied (the env's clip bound +-1).  The defaults leave every
    buffer as it was before these two existed, bit for bit (test_trained_regime_cpu.py)."""
    D, W = obs_dim, pitch(obs_dim)
    g = torch.Generator(device="cpu").manual_seed(seed)
    obs = torch.zeros((total, W))
    real = torch.rand((total, D), generator=g) * 2 - 1
    if clip_share > 0.0:
        at_bound = torch.rand((total, D), generator=torch.Generator(device="cpu").manual_seed(seed + 7919)) < clip_share
        real = torch.where(at_bound, torch.sign(real), real)
    obs[:, :D] = real * obs_scale
    Pv = views_of(flat.detach().cpu(), spec)
    with torch.no_grad():
        m0, v0 = P.mlp_forward(Pv, obs[:, :D].contiguous())
    act = m0 + torch.exp(Pv["log_std"]) * torch.randn((total, 7), generator=g)
    old_shift = 0.05 * torch.randn((total, 7), generator=g)
    if old_shift_rel:
        old_shift = old_shift * torch.exp(Pv["log_std"])
    old_logp = P.gaussian_log_prob(act, m0 + old_shift, Pv["log_std"])
    adv = torch.randn(total, generator=g) * adv_scale + adv_shift
    ret = v0 + torch.randn(total, generator=g) + ret_shift
    noise = torch.randn((total, 7), generator=g)
    return {"obs": obs, "act": act.contiguous(), "old_logp": old_logp.contiguous(), "adv": adv, "ret": ret.contiguous(), "noise": noise}


def selection(total: int, n: int, seed: int) -> torch.Tensor:
    return torch.randperm(total, generator=torch.Generator(device="cpu").manual_seed(seed))[:n].contiguous()


def reference(flat: torch.Tensor, spec, obs_dim: int, buf: dict, sel: torch.Tensor, *, clip_range: float, ent_coef: float, vf_coef: float,
              adv_mode: str, adv_stats: tuple[float, float] | None = None, dtype=torch.float64, forward=P.mlp_forward) -> dict:
    """SB3's PPO loss and its gradient through torch autograd in fp64 on the CPU.  adv_mode: "minibatch" (SB3's unbiased std), "raw" or
    "given" (mean, 1/std supplied).  Also the forward outputs of the selected rows (mean, value).  dtype = torch.float32: the same
    expressions in float32, whose distance from the fp64 result is the rounding of a plain fp32 evaluation (the e32 of the bounds);
    forward: what stands in for P.mlp_forward (tests/trained_regime.py passes one with another activation)."""
    sel = sel.cpu()
    f = flat.detach().cpu().to(dtype).clone().requires_grad_(True)
    Pv = views_of(f, spec)
    obs = buf["obs"][sel, :obs_dim].to(dtype)
    mean, value = forward(Pv, obs)
    logp = P.gaussian_log_prob(buf["act"][sel].to(dtype), mean, Pv["log_std"])
    a = buf["adv"][sel].to(dtype)
    if adv_mode == "minibatch":
        a = (a - a.mean()) / (a.std() + 1e-8)
    elif adv_mode == "given":
        a = (a - float(np.float32(adv_stats[0]))) * float(np.float32(adv_stats[1]))
    else:
        assert adv_mode == "raw"
    log_ratio = logp - buf["old_logp"][sel].to(dtype)
    ratio = torch.exp(log_ratio)
    pl = -torch.min(a * ratio, a * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    vl = torch.nn.functional.mse_loss(buf["ret"][sel].to(dtype), value)
    entropy = (0.5 + 0.5 * math.log(2 * math.pi) + Pv["log_std"]).sum()
    loss = pl + ent_coef * (-entropy) + vf_coef * vl
    (grad,) = torch.autograd.grad(loss, f)
    return {"grad": grad, "policy_loss": pl.item(), "value_loss": vl.item(), "entropy": entropy.item(), "mean": mean.detach(), "value": value.detach(),
            "frac_clipped": ((ratio - 1).abs() > clip_range).to(dtype).mean().item(), "approx_kl": ((ratio - 1) - log_ratio).mean().item()}


# ------------------------------------------------------------------------------------------------ call helpers of the GPU modules
# (shared by test_mlp_handle_state_gpu.py and test_trained_regime_gpu.py; nothing here touches a device until it is called)
DEV = torch.device("cuda", 0)
KW = dict(clip_range=0.2, ent_coef=1e-2, vf_coef=0.5)


def handle(kind, max_batch=512, replicas=1):
    from rl_brain_trainer_amd.mlp import MlpKernels

    hidden, obs_dim, path = kind
    k = MlpKernels(hidden, DEV, max_batch=max_batch, obs_dim=obs_dim, replicas=replicas)
    if hidden == 256:
        k.set_fused(path == "fused")
    return k


def dev(buf: dict) -> dict:
    return {name: t.to(DEV).contiguous() for name, t in buf.items()}


def loss_grad(k, buf: dict, idx, n: int, grad, stats, obs=None, **over):
    k.loss_grad(buf["obs"] if obs is None else obs, idx, n, buf["act"], buf["old_logp"], buf["adv"], buf["ret"], inv_count=1.0 / n, grad_out=grad,
                stats_out=stats, **{**KW, **over})


def check_kl(slot3: float, klb: dict, what, calls: int = 1) -> float:
    """stats_out[3] after `calls` accumulating calls against approx_kl = mean((ratio - 1) - log ratio) in fp64.  This comparison has no project
    tolerance; the bound is row_attribution.approx_kl_bound's 8 * max(e32, floor): e32 = the error of the same expression evaluated with
    P.mlp_forward / P.gaussian_log_prob in float32 on the CPU, floor = 2^-23 * max(1, max|logp|) * mean|log ratio| (log ratio inherits one fp32
    spacing of the log-prob, and d kl / d log ratio = ratio - 1 ~ log ratio).  The value is > 100 x the bound (also asserted by the CPU
    companions), so a missing inv_count, another slot or the second-order formula cannot pass.  Returns error / bound."""
    assert klb["kl64"] > 100 * klb["bound"], (what, klb)
    err = abs(slot3 - calls * klb["kl64"])
    assert err <= calls * klb["bound"], f"{what} approx_kl: got {slot3} for {calls} call(s) of {klb['kl64']}, error {err:.3e} bound {calls * klb['bound']:.3e}"
    return err / (calls * klb["bound"])


def norm_shares(grad: torch.Tensor, spec) -> dict[str, float]:
    """each tensor's share of the squared gradient norm, in fp64"""
    g = grad.detach().cpu().double()
    s2 = float((g * g).sum())
    return {name: float((g[sl] * g[sl]).sum()) / s2 for name, sl in slices_of(spec).items()}


# ------------------------------------------------------------------------------------------------ section 3: the clip-norm inputs
# Chosen so that on the fp64 gradient every tensor of the spec holds >= 1e-4 of the squared norm (asserted by the CPU companion and again by
# the GPU test): log_std's gradient is -ent_coef per element plus a policy-loss part, so ent_coef is order 0.1 .. 1; raw advantages with an
# offset and returns with an offset keep the bias tensors (one element for value_net.bias) above the floor; the action head is scaled so
# that the policy net's gradient does not vanish behind it.
CLIP_NORM = dict(n=200, clip_range=0.2, ent_coef=0.5, vf_coef=0.5, head_scale=60.0, adv_scale=1.0, adv_shift=0.5, ret_shift=1.0, seed=7, sel_seed=70)
MIN_SHARE = 1e-4


def clip_norm_case(hidden: int, obs_dim: int):
    c = CLIP_NORM
    pol = policy(hidden, obs_dim, head_scale=c["head_scale"])
    buf = sample_buffers(pol.flat, pol.spec, obs_dim, seed=c["seed"], adv_scale=c["adv_scale"], adv_shift=c["adv_shift"], ret_shift=c["ret_shift"])
    sel = selection(TOTAL, c["n"], c["sel_seed"])
    return pol, buf, sel


# ------------------------------------------------------------------------------------------------ section 4: Adam over several steps
ADAM = dict(lr=1e-3, eps=1e-5, max_grad_norm=0.5, ns=(200, 33, 200, 1), clip_range=0.2, ent_coef=1e-2, vf_coef=0.5, seed=9)


def adam_restatement(p0: torch.Tensor, grads: list[torch.Tensor], *, c0: int, lr: float, eps: float, max_grad_norm: float, dtype, shift: int = 0):
    """clip_grad_norm_ + torch.optim.Adam from m = v = 0, steps t = c0 + 1 + shift ...; the clip norm S_t is taken from the fp64 gradient in
    both precisions, so dtype = float32 differs from float64 by the rounding of the recurrences alone.  Returns [(p, m, v)] after each step."""
    p = p0.detach().cpu().to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    one = torch.ones((), dtype=dtype)
    out = []
    for i, g64 in enumerate(grads):
        g64 = g64.detach().cpu().double()
        t = c0 + 1 + i + shift
        S = torch.sqrt((g64 * g64).sum()).to(dtype)
        c = torch.minimum(torch.tensor(max_grad_norm, dtype=dtype) / (S + torch.tensor(1e-6, dtype=dtype)), one)
        g = g64.to(dtype) * c
        m = torch.tensor(0.9, dtype=dtype) * m + torch.tensor(0.1, dtype=dtype) * g
        v = torch.tensor(0.999, dtype=dtype) * v + torch.tensor(0.001, dtype=dtype) * g * g
        bc1 = one - torch.tensor(0.9, dtype=dtype) ** t
        bc2 = one - torch.tensor(0.999, dtype=dtype) ** t
        p = p - (torch.tensor(lr, dtype=dtype) / bc1) * (m / (v.sqrt() / bc2.sqrt() + torch.tensor(eps, dtype=dtype)))
        out.append((p.clone(), m.clone(), v.clone()))
    return out


def adam_bounds(ref64, ref32, spec) -> list[dict[str, dict[str, tuple[float, float]]]]:
    """per step, per tensor of the spec and for each of p, m, v: (e32, bound) with bound = 8 * max(e32, ulp(max|tensor|)), e32 the error of
    the fp32 recurrences against the fp64 restatement (test_anchor_step_against_fp64_restatement's idiom)"""
    out = []
    for s64, s32 in zip(ref64, ref32):
        step = {}
        for name, sl in slices_of(spec).items():
            step[name] = {}
            for what, r, f in zip("pmv", s64, s32):
                e32 = (f[sl].double() - r[sl]).abs().max().item()
                ulp = float(np.spacing(np.float32(r[sl].abs().max().item())))
                step[name][what] = (e32, 8.0 * max(e32, ulp))
        out.append(step)
    return out


def adam_errors(ref64, got, spec) -> list[dict[str, dict[str, float]]]:
    out = []
    for s64, s in zip(ref64, got):
        out.append({name: {what: (g[sl].detach().cpu().double() - r[sl]).abs().max().item() for what, r, g in zip("pmv", s64, s)}
                    for name, sl in slices_of(spec).items()})
    return out
