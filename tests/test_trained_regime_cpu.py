"""CPU companion of test_trained_regime_gpu.py: the conditions that give its checks their power, asserted on the torch references of the
very inputs the GPU tests use (tests/trained_regime.py), so they can be checked without a GPU.

  1. the defaults of S.sample_buffers still give the buffers every older test was written on, bit for bit
  2. the trained-scale inputs are what they claim: saturated and linear shares per layer, observation entries on the clip bound, ratios
     around 1 with both clip branches, an approx_kl the bound resolves
  3. at T4 a plain float32 evaluation uses <= 0.1 of every existing tolerance, so those tolerances hold unchanged there
  4. four wrong tanh forms that equal tanh for |x| <= 2 are rejected on the new inputs ...
  5. ... while on the inputs of the older tests three of them give exactly the results of tanh, and the fourth (another backward factor
     beyond |x| = 2) does so on the rows whose pre-activations stay below 2 -- the older inputs reach |z| = 2.5 .. 3.7, not 2"""
from __future__ import annotations

import math

import pytest
import torch

import mlp_handle_state as S
import row_attribution as R
import trained_regime as T
from rl_brain_trainer_amd import ppo as P

NETS = sorted({(h, d) for h, d, _ in S.KINDS})
# (hidden, obs_dim, regime, policy seed, buffer seed, replica): the nets of S.KINDS at both regimes and the replicas of the S.POP_KINDS populations
CASES = [(h, d, regime, 3, T.BUF_SEED, 0) for h, d in NETS for regime in T.REGIMES]
CASES += [(h, d, T.POP_REGIMES[r], 3 + 10 * r, T.BUF_SEED + r, r) for h, d in S.POP_KINDS for r in range(1, T.POP_K)]
CASE_IDS = [f"{h}-{d}-{regime}-r{r}" for h, d, regime, _, _, r in CASES]
RAW_NETS = {(256, 56), (256, 80), (64, 56)}        # the fused and the 2x64 kinds also run with raw advantages


def _sample_buffers_before(flat, spec, obs_dim, *, total=S.TOTAL, seed=1, adv_scale=3.0, adv_shift=0.5, ret_shift=0.0, obs_scale=1.0):
    """S.sample_buffers as it stood before old_shift_rel and clip_share, kept here as the fixed point of test 1"""
    D, W = obs_dim, S.pitch(obs_dim)
    g = torch.Generator(device="cpu").manual_seed(seed)
    obs = torch.zeros((total, W))
    obs[:, :D] = (torch.rand((total, D), generator=g) * 2 - 1) * obs_scale
    Pv = S.views_of(flat.detach().cpu(), spec)
    with torch.no_grad():
        m0, v0 = P.mlp_forward(Pv, obs[:, :D].contiguous())
    act = m0 + torch.exp(Pv["log_std"]) * torch.randn((total, 7), generator=g)
    old_logp = P.gaussian_log_prob(act, m0 + 0.05 * torch.randn((total, 7), generator=g), Pv["log_std"])
    adv = torch.randn(total, generator=g) * adv_scale + adv_shift
    ret = v0 + torch.randn(total, generator=g) + ret_shift
    noise = torch.randn((total, 7), generator=g)
    return {"obs": obs, "act": act.contiguous(), "old_logp": old_logp.contiguous(), "adv": adv, "ret": ret.contiguous(), "noise": noise}


# ================================================================================================ 1. the old buffers
@pytest.mark.parametrize("hidden,obs_dim", NETS)
def test_default_sample_buffers_are_the_old_ones_bit_for_bit(hidden, obs_dim):
    pol = S.policy(hidden, obs_dim)
    for kw in ({}, {"seed": 7, "adv_scale": 1.0, "adv_shift": 0.5, "ret_shift": 1.0}, {"seed": 11, "total": 600, "obs_scale": 5.0}):
        new, old = S.sample_buffers(pol.flat, pol.spec, obs_dim, **kw), _sample_buffers_before(pol.flat, pol.spec, obs_dim, **kw)
        assert new.keys() == old.keys()
        for name in old:
            assert torch.equal(new[name].view(torch.int32), old[name].view(torch.int32)), (kw, name)


def test_forward_parts_is_mlp_forward():
    """the forward with a replaceable activation is P.mlp_forward when the activation is torch.tanh, in both precisions"""
    pol, buf = T.case(128, 80, "T4")
    for dtype in (torch.float64, torch.float32):
        Pv, obs = S.views_of(pol.flat.to(dtype), pol.spec), buf["obs"][:200, :80].to(dtype).contiguous()
        (m, v, _), (m0, v0) = T.forward_parts(Pv, obs), P.mlp_forward(Pv, obs)
        assert torch.equal(m, m0) and torch.equal(v, v0)


# ================================================================================================ 2. the regime
@pytest.mark.parametrize("hidden,obs_dim,regime,seed,buf_seed,r", CASES, ids=CASE_IDS)
def test_trained_inputs_are_saturated_and_still_hold_a_linear_range(hidden, obs_dim, regime, seed, buf_seed, r):
    """On the fp64 activations of the rows each GPU case selects: the share of |h| > 0.999 in the second and in the first hidden layer and
    the share of |h| < 0.5 in each layer against the regime's floors; and the other conditions on the inputs.  Measured here, n = 520,
    K = 1 kinds (h2 / h1 / linear): T4 0.40 .. 0.46 / 0.06 .. 0.34 / 0.08 .. 0.10; T8 0.71 .. 0.73 / 0.33 .. 0.63 / 0.04."""
    pol, buf = T.case(hidden, obs_dim, regime, seed, buf_seed)
    D, floors = obs_dim, T.FLOORS[regime]
    real = buf["obs"][:, :D]
    assert not buf["obs"][:, D:].any() and real.abs().max().item() == 1.0                      # pad columns zero, nothing past the clip bound
    assert 0.25 < (real.abs() == 1.0).double().mean().item() < 0.35                            # the seeded 30 % on the bound
    log_std = pol.views["log_std"]
    assert -4.3 <= log_std.min().item() and log_std.max().item() <= -2.2
    for n in T.NS:
        sel = T.rows(n, r)
        sh = T.shares(T.hidden_parts(pol.flat, pol.spec, D, buf["obs"][sel]))
        ref = T.loss_reference(pol.flat, pol.spec, D, buf, sel)
        klb = R.approx_kl_bound(pol.flat, pol.spec, D, buf["obs"][sel], buf["act"][sel], buf["old_logp"][sel])
        print(f"{hidden}-{D} {regime} replica {r} n={n}: |h|>0.999 h2 {sh['h2']:.3f} h1 {sh['h1']:.3f}, |h|<0.5 {sh['linear']:.3f}, max|z| {sh['max_z']:.1f}, "
              f"frac_clipped {ref['frac_clipped']:.2f}, approx_kl {ref['approx_kl']:.2e} (bound {klb['bound']:.1e})")
        assert sh["h2"] >= floors["h2"] and sh["h1"] >= floors["h1"] and sh["linear"] >= floors["linear"], (n, sh, floors)
        assert 0.02 < ref["frac_clipped"] < 0.98, (n, ref["frac_clipped"])
        assert 1e-3 < ref["approx_kl"] < 1e-1, (n, ref["approx_kl"])
        assert ref["approx_kl"] > 100 * klb["bound"], (n, klb)                                 # S.check_kl's own condition
        assert torch.isfinite(ref["grad"]).all()


@pytest.mark.parametrize("hidden,obs_dim", NETS)
def test_saturated_inputs_drive_every_first_layer_unit_to_one(hidden, obs_dim):
    """T.saturated_buffers at n = 33: in fp64 every h1 is exactly +-1 (1 - h1^2 == 0), so the reference's W1 and b1 gradients are exactly 0;
    every value is finite and the loss terms are of ordinary size; the second layer keeps a linear range."""
    pol, buf = T.case(hidden, obs_dim, "T4", saturated=True)
    sel = T.rows(T.NS[0])
    assert torch.isfinite(buf["obs"]).all() and buf["obs"].abs().max() == torch.tensor(T.SAT_SCALE) and all(torch.isfinite(t).all() for t in buf.values())
    parts = T.hidden_parts(pol.flat, pol.spec, obs_dim, buf["obs"][sel])
    for net in parts:
        assert bool((1 - parts[net]["h1"] ** 2 == 0).all()), net
    ref = T.loss_reference(pol.flat, pol.spec, obs_dim, buf, sel)
    sl = S.slices_of(pol.spec)
    for name in sl:
        dead = name.startswith("mlp_extractor.") and ".0." in name
        assert bool((ref["grad"][sl[name]] == 0).all()) == dead, name
    assert torch.isfinite(ref["grad"]).all() and 0.02 < ref["frac_clipped"] < 0.98 and 1e-3 < ref["approx_kl"] < 1e-1
    assert ref["approx_kl"] > 100 * R.approx_kl_bound(pol.flat, pol.spec, obs_dim, buf["obs"][sel], buf["act"][sel], buf["old_logp"][sel])["bound"]
    assert T.shares(parts)["linear"] == 0.0 and (torch.cat([parts[n]["h2"].reshape(-1) for n in parts]).abs() < 0.5).double().mean().item() >= 0.03


# ================================================================================================ 3. headroom at T4
def _checks(pol, obs_dim, buf, sel, adv_mode, *, dtype=torch.float64, act=None):
    loss = T.loss_reference(pol.flat, pol.spec, obs_dim, buf, sel, dtype=dtype, act=act, adv_mode=adv_mode)
    fwd = T.forward_reference(pol.flat, pol.spec, obs_dim, buf["obs"][sel], buf["noise"][sel], dtype=dtype, act=act)
    return loss, fwd


def _all_ratios(got, ref, spec) -> dict[str, float]:
    """error / existing tolerance of every check of the GPU tests: gradient per tensor, the three losses, the five forward outputs"""
    out = T.ratios(T.loss_errors(got[0], ref[0], spec), T.loss_tolerances(ref[0], spec))
    out.update({k: (v if v == v else float("inf")) for k, v in T.forward_ratios(got[1], ref[1]).items()})
    return out


@pytest.mark.parametrize("hidden,obs_dim,regime,seed,buf_seed,r", [c for c in CASES if c[2] == "T4"], ids=[i for c, i in zip(CASES, CASE_IDS) if c[2] == "T4"])
def test_float32_uses_a_tenth_of_the_existing_tolerances_at_T4(hidden, obs_dim, regime, seed, buf_seed, r):
    """The float32 CPU restatement against fp64 under the project's tolerances (gradient per tensor 2e-4 max|ref| + 1e-7, forward rtol 1e-4 /
    atol 2e-5, log_prob 1e-4, losses 1e-4 (|x| + 1)): <= 0.1 of each, on every row count and advantage mode of the GPU tests.  Measured:
    gradient <= 0.08 (log_std, 128-80, n = 520), mean <= 0.02, value <= 0.04, log_prob <= 0.005, entropy 0.047; no check above 0.08."""
    pol, buf = T.case(hidden, obs_dim, regime, seed, buf_seed)
    for n in T.NS:
        sel = T.rows(n, r)
        for mode in ("minibatch", "raw") if (hidden, obs_dim) in RAW_NETS and r == 0 else ("minibatch",):
            rat = _all_ratios(_checks(pol, obs_dim, buf, sel, mode, dtype=torch.float32), _checks(pol, obs_dim, buf, sel, mode), pol.spec)
            worst = max(rat, key=rat.get)
            print(f"{hidden}-{obs_dim} replica {r} n={n} {mode}: float32 error / tolerance, worst {rat[worst]:.3f} ({worst}), mean {rat['mean']:.3f}, "
                  f"value {rat['value']:.3f}, log_prob {rat['log_prob']:.4f}")
            assert rat[worst] <= 0.1, (n, mode, worst, rat[worst])


# ================================================================================================ 4. wrong activations are rejected
@pytest.mark.parametrize("hidden,obs_dim", NETS)
def test_wrong_activations_are_rejected_on_the_trained_inputs(hidden, obs_dim):
    """fp64 with a wrong activation in place of the device: forms a, b and c leave at least one check >= 10 existing tolerances from the
    fp64 reference at T4 (n = 520), on every net -- none needed the T8 inputs for that; form d never meets |x| > 44 at T4 (max |z| ~ 22),
    is non-finite at T8 (n = 520, max |z| > 44 on every net) and in the saturated case."""
    pol, buf = T.case(hidden, obs_dim, "T4")
    sel = T.rows(T.NS[1])
    ref = _checks(pol, obs_dim, buf, sel, "minibatch")
    for name, act in T.WRONG_TANH.items():
        rat = _all_ratios(_checks(pol, obs_dim, buf, sel, "minibatch", act=act), ref, pol.spec)
        worst = max(rat, key=rat.get)
        print(f"{hidden}-{obs_dim} T4 {name}: worst error / tolerance {rat[worst]:.1f} ({worst})")
        if name.startswith("d"):
            assert rat[worst] == 0.0
        else:
            assert rat[worst] >= 10.0, (name, rat)
    dead = T.WRONG_TANH["d: NaN beyond 44"]
    pol8, buf8 = T.case(hidden, obs_dim, "T8")
    assert T.shares(T.hidden_parts(pol8.flat, pol8.spec, obs_dim, buf8["obs"][sel]))["max_z"] > 44
    pols, bufs = T.case(hidden, obs_dim, "T4", saturated=True)
    for what, (p, b, s) in {"T8": (pol8, buf8, sel), "saturated": (pols, bufs, T.rows(T.NS[0]))}.items():
        loss, fwd = _checks(p, obs_dim, b, s, "minibatch", act=dead)
        assert not torch.isfinite(loss["grad"]).all(), what                       # (which net meets |z| > 44 first depends on the kind)
        assert not (torch.isfinite(fwd["mean"]).all() and torch.isfinite(fwd["value"]).all()), what
        assert not (math.isfinite(loss["policy_loss"]) and math.isfinite(loss["value_loss"])), what


# ================================================================================================ 5. ... and invisible before
@pytest.mark.parametrize("hidden,obs_dim", NETS)
def test_wrong_activations_are_invisible_on_the_old_inputs(hidden, obs_dim):
    """S.policy / S.sample_buffers are the inputs of every older comparison with an outside reference.  On their whole 512-row buffer no
    hidden unit passes |h| = 0.999 and no pre-activation passes 4 (measured: rms |z| 0.45 .. 0.78, max |z| 2.5 and 2.7 on the 2x256 nets,
    3.4 on 2x128 and 3.7 on 2x64), so forms a, b and d give the gradient, the losses and the forward outputs of tanh itself, bit for bit:
    the older suite could not tell them from the kernel's.
    Form c changes the backward factor beyond |x| = 2, and 0.002 % (2x256, 56) to 1 % (2x64) of the old pre-activations lie there.  It is tanh
    bit for bit on the rows none of whose pre-activations passes 2 (39 .. 499 of the 512), which is asserted; on a 200-row selection of all
    rows it stays below the gradient tolerance on 256-56 (0.7 of it) and is 20 .. 35 tolerances off on the other three nets.  So the
    older suite did hold the backward factor up to |h| ~ 0.998 on those nets; what it never met is |h| > 0.999."""
    pol = S.policy(hidden, obs_dim)
    buf = S.sample_buffers(pol.flat, pol.spec, obs_dim, seed=1)
    parts = T.hidden_parts(pol.flat, pol.spec, obs_dim, buf["obs"])
    sh = T.shares(parts)
    row_max = torch.stack([parts[n][z].abs().max(dim=1).values for n in parts for z in ("z1", "z2")]).max(dim=0).values
    inside = torch.nonzero(row_max <= 2.0).reshape(-1)
    print(f"{hidden}-{obs_dim} old inputs: max|z| {sh['max_z']:.3f}, share |h| > 0.999: h1 {sh['h1']}, h2 {sh['h2']}, rows with every |z| <= 2: {inside.numel()}")
    assert sh["max_z"] < 4.0 and sh["h1"] == 0.0 and sh["h2"] == 0.0 and inside.numel() >= 33
    sel = S.selection(S.TOTAL, 200, 70)
    kw = dict(clip_range=0.2, ent_coef=1e-2, vf_coef=0.5)
    for name, act in T.WRONG_TANH.items():
        rows = inside if name.startswith("c") else sel
        got, ref = _checks_old(pol, obs_dim, buf, rows, act, kw), _checks_old(pol, obs_dim, buf, rows, None, kw)
        for k, v in ref.items():
            assert torch.equal(torch.as_tensor(got[k]), torch.as_tensor(v)), (name, k)
        if name.startswith("c"):
            full, ref = T.loss_reference(pol.flat, pol.spec, obs_dim, buf, sel, act=act, **kw), T.loss_reference(pol.flat, pol.spec, obs_dim, buf, sel, **kw)
            rat = T.ratios(T.loss_errors(full, ref, pol.spec), T.loss_tolerances(ref, pol.spec))
            print(f"{hidden}-{obs_dim} old inputs, {name}, all rows: worst error / tolerance {max(rat.values()):.2f} ({max(rat, key=rat.get)})")


def _checks_old(pol, obs_dim, buf, sel, act, kw) -> dict:
    loss = T.loss_reference(pol.flat, pol.spec, obs_dim, buf, sel, act=act, **kw)
    fwd = T.forward_reference(pol.flat, pol.spec, obs_dim, buf["obs"][sel], buf["noise"][sel], act=act)
    return {**{k: loss[k] for k in ("grad", "policy_loss", "value_loss", "approx_kl")}, **fwd}
