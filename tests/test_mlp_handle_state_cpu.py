"""CPU companion of test_mlp_handle_state_gpu.py: the two conditions that give its optimiser checks their power, asserted on the torch fp64
reference of the very inputs the GPU tests use (tests/mlp_handle_state.py), so they can be checked without a GPU."""
from __future__ import annotations

import math

import pytest
import torch

import mlp_handle_state as S


@pytest.mark.parametrize("hidden,obs_dim", sorted({(h, d) for h, d, _ in S.KINDS}))
def test_every_tensor_carries_weight_in_the_clip_norm(hidden, obs_dim):
    """Section 3's condition: on the fp64 gradient every tensor of the spec holds >= 1e-4 of S^2.  Leaving one tensor (or, for 2x64, the
    zero-padded half of the layout, which holds none of it) out of the norm then moves the clip coefficient c = M / (S + 1e-6) by a relative
    1 - sqrt(1 - 1e-4) >= 5e-5, a hundred times the GPU test's bound of 8 * 2^-24 = 4.8e-7."""
    c = S.CLIP_NORM
    pol, buf, sel = S.clip_norm_case(hidden, obs_dim)
    ref = S.reference(pol.flat, pol.spec, obs_dim, buf, sel, clip_range=c["clip_range"], ent_coef=c["ent_coef"], vf_coef=c["vf_coef"], adv_mode="minibatch")
    shares = S.norm_shares(ref["grad"], pol.spec)
    print({k: f"{v:.2e}" for k, v in shares.items()})
    assert abs(sum(shares.values()) - 1.0) < 1e-12
    assert min(shares.values()) >= S.MIN_SHARE, min(shares.items(), key=lambda kv: kv[1])
    assert 0.02 < ref["frac_clipped"] < 0.98                      # both branches of the surrogate
    assert 1.0 - math.sqrt(1.0 - S.MIN_SHARE) >= 100 * 8 * 2.0 ** -24


def _adam_case(hidden, obs_dim):
    a = S.ADAM
    pol = S.policy(hidden, obs_dim)
    buf = S.sample_buffers(pol.flat, pol.spec, obs_dim, seed=a["seed"])
    grads = []
    for i, n in enumerate(a["ns"]):
        sel = S.selection(S.TOTAL, n, 90 + i)
        mode = "minibatch" if n > 1 else "raw"
        grads.append(S.reference(pol.flat, pol.spec, obs_dim, buf, sel, clip_range=a["clip_range"], ent_coef=a["ent_coef"], vf_coef=a["vf_coef"],
                                 adv_mode=mode)["grad"].float())
    return pol, grads


@pytest.mark.parametrize("hidden,obs_dim", [(256, 56), (64, 56)])
def test_a_step_count_off_by_one_breaks_the_adam_bound(hidden, obs_dim):
    """Section 4's condition, the fp32 torch recurrences standing in for the device: from c0 = 0 they meet the bound 8 * max(e32, ulp) by
    construction, and the same recurrences with every t shifted by +1 or by -1 (what a device counter that is off by one would compute)
    violate it on p for every weight tensor, at every one of the four steps."""
    a = S.ADAM
    kw = dict(c0=0, lr=a["lr"], eps=a["eps"], max_grad_norm=a["max_grad_norm"])
    pol, grads = _adam_case(hidden, obs_dim)
    ref64 = S.adam_restatement(pol.flat, grads, dtype=torch.float64, **kw)
    ref32 = S.adam_restatement(pol.flat, grads, dtype=torch.float32, **kw)
    bounds = S.adam_bounds(ref64, ref32, pol.spec)
    for shift in (+1, -1):
        err = S.adam_errors(ref64, S.adam_restatement(pol.flat, grads, dtype=torch.float32, shift=shift, **kw), pol.spec)
        for step, (e, b) in enumerate(zip(err, bounds)):
            for name, _ in pol.spec:
                if name.endswith("weight"):
                    assert not e[name]["p"] <= b[name]["p"][1], (shift, step, name, e[name]["p"], b[name]["p"])
    # and c0 = 1000 is a different trajectory from c0 = 0 (what the GPU test asserts of the device there)
    far = S.adam_restatement(pol.flat, grads, dtype=torch.float64, **{**kw, "c0": 1000})
    assert all((f[0] != r[0]).any() for f, r in zip(far, ref64))
