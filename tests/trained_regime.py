"""Shared by test_trained_regime_gpu.py, test_trained_regime_cpu.py and the trained-scale cases of the one-launch parity modules: policies
at the scale of a policy after 1 .. 12 G steps (a large share of saturated tanh units, log_std of -2 .. -4), sample buffers with observation
entries on the +-1 clip bound, the fp64 / fp32 references and the bounds of the comparison.  Everything here is plain torch on the CPU, in
the idiom of tests/mlp_handle_state.py, whose policy, buffers and reference it extends and does not restate."""
from __future__ import annotations

import functools

import torch

import mlp_handle_state as S
import row_attribution as R
from rl_brain_trainer_amd import ppo as P

# regime -> factors on mlp_handle_state.policy: hidden weights, hidden biases, the action head, and the shift of log_std
REGIMES = {"T4": dict(weight=4.0, bias=5.0, head=30.0, log_std=-2.5), "T8": dict(weight=8.0, bias=5.0, head=30.0, log_std=-3.5)}
# floors of the CPU companion, per regime: share of |h| > 0.999 in the second and in the first hidden layer, share of |h| < 0.5 in each
FLOORS = {"T4": dict(h2=0.3, h1=0.05, linear=0.03), "T8": dict(h2=0.6, h1=0.3, linear=0.03)}
TOTAL = 1024                    # rows of every buffer; the selections are gathered from it
NS = (33, 520)                  # a one-row second tile; past 512 with ragged last chunks on both paths (row_attribution.units)
LOSS = dict(clip_range=0.1, ent_coef=1e-3, vf_coef=0.5)
CLIP_SHARE = 0.3
SAT_SCALE = 1e18
POP_K = 3
POP_REGIMES = ("T4", "T8", "T4")
# Buffer seed of replica 0 (replica r: BUF_SEED + r).  Of the seeds 1 .. 4 this is the one at which the float32 CPU restatement stays below
# 0.1 of every existing tolerance at T4 on every kind, both row counts and both advantage modes (the CPU companion asserts it): a choice made
# on the CPU reference's own rounding, never on the kernels' results.
BUF_SEED = 4
# the project's tolerances for a comparison with fp64: forward outputs (rtol, atol); the gradient's is row_attribution.tolerances
FWD_TOL = {"mean": (1e-4, 2e-5), "value": (1e-4, 2e-5), "action": (1e-4, 2e-5), "clipped": (1e-4, 2e-5), "log_prob": (1e-4, 1e-4)}
LOSS_TOL = {"policy_loss": lambda x: 1e-4 * (abs(x) + 1), "value_loss": lambda x: 1e-4 * (abs(x) + 1), "entropy": lambda x: 1e-5}


def trained_policy(hidden: int, obs_dim: int, regime: str, seed: int = 3) -> P.ActorCritic:
    pol = S.policy(hidden, obs_dim, seed=seed)
    r = REGIMES[regime]
    for name, _ in pol.spec:
        if name.startswith("mlp_extractor."):
            pol.views[name].mul_(r["weight"] if name.endswith("weight") else r["bias"])
    pol.views["action_net.weight"].mul_(r["head"])
    pol.views["log_std"].copy_(torch.tensor(S.LOG_STD) + r["log_std"])
    return pol


def trained_buffers(flat: torch.Tensor, spec, obs_dim: int, *, seed: int = BUF_SEED, total: int = TOTAL, obs_scale: float = 1.0) -> dict[str, torch.Tensor]:
    """S.sample_buffers with 30 % of the real observation entries on the clip bound and the old policy's mean shifted by 0.05 sigma randn"""
    return S.sample_buffers(flat, spec, obs_dim, total=total, seed=seed, obs_scale=obs_scale, old_shift_rel=True, clip_share=CLIP_SHARE)


def saturated_buffers(flat: torch.Tensor, spec, obs_dim: int, *, seed: int = BUF_SEED, total: int = TOTAL) -> dict[str, torch.Tensor]:
    """trained_buffers' rows with the real observation columns times 1e18 (finite, and no product of the network overflows): every
    non-zero pre-activation of layer 1 saturates.  Actions, old log-probs and returns are those of the policy on these observations."""
    return trained_buffers(flat, spec, obs_dim, seed=seed, total=total, obs_scale=SAT_SCALE)


@functools.lru_cache(maxsize=None)
def case(hidden: int, obs_dim: int, regime: str, seed: int = 3, buf_seed: int = BUF_SEED, saturated: bool = False):
    """(policy, buffers) of one net; computed once, shared by every test that needs it and modified by none"""
    pol = trained_policy(hidden, obs_dim, regime, seed)
    build = saturated_buffers if saturated else trained_buffers
    return pol, build(pol.flat, pol.spec, obs_dim, seed=buf_seed)


def rows(n: int, r: int = 0) -> torch.Tensor:
    """the n rows of the 1024-row buffer that replica r selects"""
    return S.selection(TOTAL, n, 2000 + 10 * n + r)


@functools.lru_cache(maxsize=None)
def population(hidden: int, obs_dim: int):
    """K = 3 replicas, each with its own seed and its own 1024 rows of one [3 * 1024]-row buffer; regimes T4, T8, T4.
    -> ([policy], {name: [3 * 1024, ...]})"""
    cases = [case(hidden, obs_dim, POP_REGIMES[r], seed=3 + 10 * r, buf_seed=BUF_SEED + r) for r in range(POP_K)]
    return [c[0] for c in cases], {name: torch.cat([c[1][name] for c in cases]).contiguous() for name in cases[0][1]}


# ------------------------------------------------------------------------------------------------ forward with a replaceable activation
def forward_parts(Pv: dict[str, torch.Tensor], obs: torch.Tensor, act=torch.tanh):
    """P.mlp_forward with the activation as an argument -> (mean, value, {net: {z1, h1, z2, h2}}).  With torch.tanh it is P.mlp_forward
    bit for bit (asserted by the CPU companion)."""
    parts, top = {}, {}
    for net in ("policy_net", "value_net"):
        pre = f"mlp_extractor.{net}."
        z1 = torch.addmm(Pv[pre + "0.bias"], obs, Pv[pre + "0.weight"].t())
        h1 = act(z1)
        z2 = torch.addmm(Pv[pre + "2.bias"], h1, Pv[pre + "2.weight"].t())
        h2 = act(z2)
        parts[net], top[net] = {"z1": z1, "h1": h1, "z2": z2, "h2": h2}, h2
    mean = torch.addmm(Pv["action_net.bias"], top["policy_net"], Pv["action_net.weight"].t())
    value = torch.addmm(Pv["value_net.bias"], top["value_net"], Pv["value_net.weight"].t()).squeeze(-1)
    return mean, value, parts


def forward_with(act):
    return lambda Pv, obs: forward_parts(Pv, obs, act)[:2]


def hidden_parts(flat: torch.Tensor, spec, obs_dim: int, obs_rows: torch.Tensor) -> dict:
    """the fp64 pre-activations and activations of the given observation rows"""
    with torch.no_grad():
        return forward_parts(S.views_of(flat.detach().cpu().double(), spec), obs_rows[:, :obs_dim].double())[2]


def shares(parts: dict) -> dict[str, float]:
    """over both nets: share of |h| > 0.999 per layer, and the smaller of the two layers' shares of |h| < 0.5"""
    h1 = torch.cat([parts[n]["h1"].reshape(-1) for n in parts]).abs()
    h2 = torch.cat([parts[n]["h2"].reshape(-1) for n in parts]).abs()
    return {"h1": (h1 > 0.999).double().mean().item(), "h2": (h2 > 0.999).double().mean().item(),
            "linear": min((h1 < 0.5).double().mean().item(), (h2 < 0.5).double().mean().item()),
            "max_z": max(parts[n][z].abs().max().item() for n in parts for z in ("z1", "z2"))}


# ------------------------------------------------------------------------------------------------ references
def loss_reference(pol_flat: torch.Tensor, spec, obs_dim: int, buf: dict, sel: torch.Tensor, *, dtype=torch.float64, act=None, adv_mode: str = "minibatch",
                   **loss) -> dict:
    """S.reference at the loss settings of these tests, in `dtype`, optionally with another activation"""
    kw = {**LOSS, **loss}
    return S.reference(pol_flat, spec, obs_dim, buf, sel, adv_mode=adv_mode, dtype=dtype, forward=P.mlp_forward if act is None else forward_with(act), **kw)


def forward_reference(pol_flat: torch.Tensor, spec, obs_dim: int, obs_rows: torch.Tensor, noise_rows: torch.Tensor, *, dtype=torch.float64, act=None) -> dict:
    """the five outputs of MlpKernels.forward for the given rows: action = mean + sigma * noise, clipped to [-1, 1], and the log-prob of
    that action computed from the noise, sum(-noise^2 / 2 - log_std - log sqrt(2 pi)), as the kernel computes it"""
    Pv = S.views_of(pol_flat.detach().cpu().to(dtype), spec)
    with torch.no_grad():
        mean, value = (P.mlp_forward if act is None else forward_with(act))(Pv, obs_rows[:, :obs_dim].to(dtype).contiguous())
        z = noise_rows.to(dtype)
        action = mean + torch.exp(Pv["log_std"]) * z
        logp = (-0.5 * z * z - Pv["log_std"] - P.LOG_SQRT_2PI).sum(-1)
    return {"mean": mean, "value": value, "action": action, "clipped": action.clamp(-1.0, 1.0), "log_prob": logp}


def assert_step_against_fp64(flat: torch.Tensor, hidden: int, obs_dim: int, obs: torch.Tensor, noise: torch.Tensor | None, got: dict, what) -> None:
    """One step of a one-launch kernel (K = 1) against an fp64 forward of the observations the env held at that step, under the forward
    tolerances.  got: some of value / log_prob / action (unclipped) / clipped; noise None: the deterministic action, got = {"clipped": ...}"""
    obs = obs.detach().cpu()
    noise = torch.zeros((obs.shape[0], 7)) if noise is None else noise.detach().cpu()
    rat = forward_ratios(got, forward_reference(flat, P.param_spec(hidden, obs_dim), obs_dim, obs, noise))
    print(f"{what} against fp64, error / tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in rat.items()))
    assert rat and max(rat.values()) <= 1.0, (what, rat)


# ------------------------------------------------------------------------------------------------ error / bound
def _flat64(t) -> torch.Tensor:
    return t.detach().cpu().double()


def loss_errors(got: dict, ref: dict, spec) -> dict[str, float]:
    """max |got - fp64| per tensor of the gradient and for the three losses.  got: {"grad": [P], "policy_loss", "value_loss", "entropy"}"""
    g, r = _flat64(got["grad"]), ref["grad"]
    out = {name: (g[sl] - r[sl]).abs().max().item() for name, sl in S.slices_of(spec).items()}
    out.update({name: abs(float(got[name]) - ref[name]) for name in LOSS_TOL})
    return out


def loss_tolerances(ref: dict, spec) -> dict[str, float]:
    """the project's tolerances: gradient per tensor 2e-4 * max|ref| + 1e-7, losses 1e-4 * (|x| + 1), entropy 1e-5"""
    out = R.tolerances(ref["grad"], spec)
    out.update({name: tol(ref[name]) for name, tol in LOSS_TOL.items()})
    return out


def forward_ratios(got: dict, ref: dict, e32: dict | None = None) -> dict[str, float]:
    """per output: max over the elements of |got - fp64| / max(atol + rtol |fp64|, 8 e32), e32 the output's largest fp32-restatement
    error (None: the project's tolerance alone)"""
    out = {}
    for name, (rtol, atol) in FWD_TOL.items():
        if name not in got:
            continue
        bound = atol + rtol * ref[name].abs()
        if e32 is not None:
            bound = bound.clamp_min(8.0 * e32[name])
        out[name] = ((_flat64(got[name]).reshape(ref[name].shape) - ref[name]).abs() / bound).max().item()
    return out


def forward_errors(got: dict, ref: dict) -> dict[str, float]:
    return {name: (_flat64(got[name]).reshape(ref[name].shape) - ref[name]).abs().max().item() for name in FWD_TOL if name in got}


def ratios(err: dict[str, float], tol: dict[str, float], e32: dict[str, float] | None = None) -> dict[str, float]:
    """error / bound; bound = the project's tolerance (T4), or max(tolerance, 8 e32) where the fp32 restatement's error is given (T8: the
    idiom of S.adam_bounds and R.approx_kl_bound).  A non-finite error gives inf."""
    out = {}
    for name, e in err.items():
        bound = tol[name] if e32 is None else max(tol[name], 8.0 * e32[name])
        out[name] = e / bound if e == e else float("inf")
    return out


# ------------------------------------------------------------------------------------------------ wrong activations
class _HalfBackward(torch.autograd.Function):
    """tanh whose backward factor is 1 - |h|"""

    @staticmethod
    def forward(ctx, x):
        h = torch.tanh(x)
        ctx.save_for_backward(h)
        return h

    @staticmethod
    def backward(ctx, g):
        (h,) = ctx.saved_tensors
        return g * (1 - h.abs())


def _wrong_backward(x):
    far = x.abs() > 2
    return torch.where(far, _HalfBackward.apply(x), torch.tanh(x))


# each is tanh itself for |x| <= 2, value and derivative
WRONG_TANH = {
    "a: +-1 beyond 4": lambda x: torch.where(x.abs() > 4, torch.sign(x), torch.tanh(x)),
    "b: argument clamped to +-4": lambda x: torch.tanh(x.clamp(-4.0, 4.0)),
    "c: backward factor 1 - |h| beyond 2": _wrong_backward,
    "d: NaN beyond 44": lambda x: torch.where(x.abs() > 44, torch.full_like(x, float("nan")), torch.tanh(x)),
}
