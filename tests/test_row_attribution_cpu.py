"""CPU companion of test_row_attribution_gpu.py and of the approx_kl assertions: the conditions that give those GPU checks their power,
asserted on the fp64 torch references of the very inputs the GPU tests use (tests/row_attribution.py, tests/mlp_handle_state.py)."""
from __future__ import annotations

import math

import pytest
import torch

import mlp_handle_state as S
import row_attribution as R

# what the references depend on: (hidden, obs_dim, gather, K); the GPU module runs the five handle kinds on them
CASES = [(h, d, gather, 1) for h, d in sorted({(h, d) for h, d, _ in S.KINDS}) for gather in (True, False)] + [(h, d, True, 3) for h, d in S.POP_KINDS]
IDS = [f"{h}-{d}-{'idx' if gather else 'prefix'}-K{K}" for h, d, gather, K in CASES]
_cache: dict = {}


def _case(hidden, obs_dim, gather, K):
    key = (hidden, obs_dim, gather, K)
    if key not in _cache:
        c = R.build(hidden, obs_dim, gather=gather, K=K)
        c["sides"] = {"policy": (R.policy_side(c), 0.0), "value": (R.value_side(c), R.VF_COEF)}
        c["teacher"] = R.anchor_side(c) if hidden != 256 else None
        _cache[key] = c
    return _cache[key]


def _sides(c):
    """(side, r, reference over given rows) for every side and replica of the case"""
    for side, (buf, vf) in c["sides"].items():
        for r in range(c["K"]):
            yield side, r, (lambda rows, count=R.NS, buf=buf, vf=vf, r=r: R.loss_reference(c, buf, r, rows, vf, count)["grad"])
    if c["teacher"] is not None:
        for r in range(c["K"]):
            yield "anchor", r, (lambda rows, count=None, r=r: R.anchor_reference(c, c["teacher"], r, rows)["grad"])


@pytest.mark.parametrize("hidden,obs_dim,gather,K", CASES, ids=IDS)
def test_every_spike_row_is_inside_the_clip_range(hidden, obs_dim, gather, K):
    """fp64 ratio of every spike row in (1 - clip, 1 + clip), with room: |log ratio| <= 0.1 + one fp32 spacing of old_logp.  A clipped row
    would carry no policy gradient and its position would go unchecked."""
    c = _case(hidden, obs_dim, gather, K)
    rows = c["spike_rows"].reshape(-1)
    assert rows.numel() == K * R.NS and rows.unique().numel() == rows.numel()
    lr = c["logp64"][rows] - c["old_logp"][rows].double()
    assert lr.abs().max().item() <= 0.1 + 1e-5 and math.exp(0.1 + 1e-5) < 1 + R.CLIP_RANGE and math.exp(-0.1 - 1e-5) > 1 - R.CLIP_RANGE
    assert (c["sides"]["policy"][0]["adv"][rows].abs() >= 1.0).all() and (c["sides"]["policy"][0]["adv"][c["silent"]] == 0).all()
    assert int(c["silent"].sum()) == K * (R.N - R.NS)


@pytest.mark.parametrize("hidden,obs_dim,gather,K", CASES, ids=IDS)
def test_silent_rows_contribute_nothing_in_fp64(hidden, obs_dim, gather, K):
    """The fp64 gradient of the whole 2065-row minibatch, silent rows included, against the gradient over S alone, both scaled by 1 / |S| as
    the kernel is: equal to <= 1e-5 of each tensor's scale (policy side: exactly; value and anchor side: the returns / teacher actions of
    the silent rows are the fp64 outputs rounded to fp32).  The tensors of the side that is switched off are exactly zero in both."""
    c = _case(hidden, obs_dim, gather, K)
    for side, r, ref in _sides(c):
        full, only = ref(c["idx"][r]), ref(c["spike_rows"][r])
        on = R.active(side)
        worst = 0.0
        for name, sl in S.slices_of(c["spec"]).items():
            if not on(name):
                assert not full[sl].any() and not only[sl].any(), (side, r, name)
                continue
            scale = only[sl].abs().max().item()
            assert scale > 0, (side, r, name)
            worst = max(worst, (full[sl] - only[sl]).abs().max().item() / scale)
        print(f"{side} replica {r}: full batch vs S alone, worst difference / scale {worst:.2e}")
        assert worst <= 1e-5, (side, r, worst)


@pytest.mark.parametrize("hidden,obs_dim,gather,K", CASES, ids=IDS)
def test_leaving_one_spike_out_breaks_the_tolerance_tenfold(hidden, obs_dim, gather, K):
    """For every spike row j: the reference over S without j differs from the reference over S, in at least one tensor of the active net, by
    >= 10 x that tensor's tolerance (2e-4 * max|ref| + 1e-7).  The loss is a sum over rows, so that difference is row j's own gradient / |S|.
    A kernel that drops row j, counts it twice or credits it to another replica is then off by >= 10 tolerances."""
    c = _case(hidden, obs_dim, gather, K)
    for side, r, ref in _sides(c):
        tol = R.tolerances(ref(c["spike_rows"][r]), c["spec"])
        on = R.active(side)
        weakest = math.inf
        for j, p in enumerate(R.POSITIONS):
            gj = ref(c["spike_rows"][r][j:j + 1])
            seen = max(gj[sl].abs().max().item() / tol[name] for name, sl in S.slices_of(c["spec"]).items() if on(name))
            assert seen >= 10.0, (side, r, p, seen)
            weakest = min(weakest, seen)
        print(f"{side} replica {r}: weakest leave-one-out change / tolerance {weakest:.1f}")


@pytest.mark.parametrize("kind", S.KINDS, ids=S.KIND_IDS)
def test_positions_cover_every_boundary_of_the_launch(kind):
    """POSITIONS holds the first and the last row, and the row before and the row at the first and the last boundary of every partition of
    the batch that the launch code makes at n = 2065 (R.units restates it), for the loss kernels and for the anchor step."""
    expect = {"fused": [8, 32, 320, 192], "layer": [32, 64, 128 if kind[0] == 256 else 64, 64]}[kind[2]]
    assert list(R.units(kind, R.N).values()) == expect
    assert 0 in R.POSITIONS and R.N - 1 in R.POSITIONS and len(set(R.POSITIONS)) == R.NS == len(R.BOUNDARY_POSITIONS) + 3
    forms = [False] + ([True] if kind in R.ANCHOR_KINDS else [])
    for anchor in forms:
        for name, (first, last) in R.boundaries(kind, R.N, anchor).items():
            assert 0 < first <= last < R.N
            for p in (first - 1, first, last - 1, last):
                assert p in R.POSITIONS, (kind, anchor, name, p)
    assert R.N <= R.MAX_BATCH and R.tn_chunk_rows(129, 8) == 64 and R.tn_chunk_rows(2065, 8) == 128


# ------------------------------------------------------------------------------------------------ approx_kl
def _edge_inputs():
    import test_mlp_handle_state_gpu as G     # its case list and hyper-parameters; importing it touches no GPU

    seen = {}
    for kind, n, max_batch in G.EDGE_CASES:
        seen.setdefault((kind[0], kind[1], n, max(S.TOTAL, max_batch)), None)
    return list(seen)


@pytest.mark.parametrize("hidden,obs_dim,n,total", _edge_inputs())
def test_approx_kl_is_far_above_its_bound_on_the_edge_inputs(hidden, obs_dim, n, total):
    """On the inputs of test_batch_size_edges_against_fp64_autograd: approx_kl in fp64 > 100 x the bound the GPU test holds stats_out[3] to.
    A kernel that forgot inv_count (n times too large), wrote another slot (0 where approx_kl belongs) or used the second-order form
    mean(log ratio^2) / 2 (off by about mean(log ratio^3) / 6, a few percent) is then outside it."""
    pol = S.policy(hidden, obs_dim)
    buf = S.sample_buffers(pol.flat, pol.spec, obs_dim, total=total, seed=11)
    sel = S.selection(total, n, 1000 + n)
    b = R.approx_kl_bound(pol.flat, pol.spec, obs_dim, buf["obs"][sel], buf["act"][sel], buf["old_logp"][sel])
    ref = S.reference(pol.flat, pol.spec, obs_dim, buf, sel, clip_range=0.2, ent_coef=1e-2, vf_coef=0.5, adv_mode="raw")
    assert ref["approx_kl"] == pytest.approx(b["kl64"], rel=1e-12)
    print(f"n={n}: approx_kl {b['kl64']:.4e} e32 {b['e32']:.2e} floor {b['floor']:.2e} bound {b['bound']:.2e} kl / bound {b['kl64'] / b['bound']:.0f}")
    assert b["kl64"] > 100 * b["bound"], b
    # what those kernels would leave in slot 3, spelled out: each is outside the bound
    wrong = {"inv_count missing": n * b["kl64"], "inv_count applied twice": b["kl64"] / n, "another slot": 0.0, "second order": b["second_order64"]}
    for what, value in wrong.items():
        if n > 1 or what in ("another slot", "second order"):
            assert abs(value - b["kl64"]) > b["bound"], (what, value, b)


@pytest.mark.parametrize("hidden,obs_dim", S.POP_KINDS)
def test_population_approx_kl_references_differ_and_clear_their_bounds(hidden, obs_dim):
    """the n = 33 probe of test_population_probe_is_independent_of_history_and_matches_single_handles: three policies on one sample buffer,
    each replica its own rows -- the three fp64 values are pairwise further apart than their bounds, and each > 100 x its bound"""
    pols = [S.policy(hidden, obs_dim, seed=3 + 10 * r) for r in range(3)]
    buf = S.sample_buffers(pols[0].flat, pols[0].spec, obs_dim, seed=1)
    out = []
    for r, pol in enumerate(pols):
        sel = S.selection(S.TOTAL, 33, 100 + r)
        out.append(R.approx_kl_bound(pol.flat, pol.spec, obs_dim, buf["obs"][sel], buf["act"][sel], buf["old_logp"][sel]))
        print(f"replica {r}: approx_kl {out[-1]['kl64']:.4e} bound {out[-1]['bound']:.2e}")
        assert out[-1]["kl64"] > 100 * out[-1]["bound"], (r, out[-1])
    for a in range(3):
        for b in range(a + 1, 3):
            assert abs(out[a]["kl64"] - out[b]["kl64"]) > out[a]["bound"] + out[b]["bound"], (a, b)
