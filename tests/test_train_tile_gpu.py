"""KP1_MLP_OPT_TRAIN_TILE on the MI355X: kp1_mlp_loss_grad of a hidden 64 / 128 handle as one tile launch
(train_tile128_kernel) + grad_finalize, against the layer-wise launches of the same handle (bit for bit where both sum the same 32-row
block records) and against fp64 torch autograd on the CPU under the project's existing rules:

    fresh policies, T4, saturated:  trained_regime.loss_tolerances (gradient per tensor 2e-4 max|ref| + 1e-7, losses 1e-4 (|x| + 1))
    T8:                             max(that tolerance, 8 e32), e32 = |float32 torch on the CPU - fp64| on the same rows

Row counts: 1 (a lone row), 31, 33 (a one-row second tile), 96 (whole tiles), 520 (17 tiles, the last with 8 rows); every selection is a
permutation with repeated rows.  KP1_TRAIN_TILE_OUT=<file>: error / bound of both paths, side by side, is written there."""
from __future__ import annotations

import ctypes as C
import json
import os

import pytest
import torch

import mlp_handle_state as S
import row_attribution as R
import trained_regime as T
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd.mlp import _p

pytestmark = pytest.mark.gpu
DEV = S.DEV
NAN = float("nan")
KINDS = [(64, 56, "layer"), (128, 80, "layer")]
KIND_IDS = ["64-56", "128-80"]
NS = (1, 31, 33, 96, 520)
MAX_BATCH = 1024
TOTAL = T.TOTAL
# the gradient tensors that are sums of hpart records (one per 32-row block on both paths): bit-equal to the layer-wise result
HPART = ("log_std", "action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias", "mlp_extractor.policy_net.2.bias",
         "mlp_extractor.value_net.2.bias")
KP1_ERR_UNSUPPORTED = -4     # include/kp1.h
_RATIOS: dict[str, dict[str, dict[str, float]]] = {}      # case -> path -> check -> error / bound


@pytest.fixture(scope="module")
def world():
    """per (kind, K): one handle reused by every case, as training reuses it; per key: buffers on the device"""
    handles, bufs = {}, {}

    def get_handle(kind, K=1, max_batch=MAX_BATCH):
        key = (kind, K, max_batch)
        if key not in handles:
            handles[key] = S.handle(kind, max_batch=max_batch, replicas=K)
        handles[key].set_train_tile(False)
        return handles[key]

    def get_buf(key, buf):
        if key not in bufs:
            bufs[key] = S.dev(buf)
        return bufs[key]

    yield get_handle, get_buf
    for k in handles.values():
        k.close()
    out = os.environ.get("KP1_TRAIN_TILE_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(_RATIOS, f, indent=1, sort_keys=True)


def _rows(n: int, r: int = 0) -> torch.Tensor:
    """T.rows(n, r) with repeats: every seventh position from 1 on holds the row of position 0"""
    sel = T.rows(n, r).clone()
    sel[1::7] = sel[0]
    return sel


def _fresh(hidden: int, obs_dim: int):
    pol = S.policy(hidden, obs_dim)
    return pol, _fresh_buffers(hidden, obs_dim)


_FRESH: dict = {}


def _fresh_buffers(hidden: int, obs_dim: int):
    if (hidden, obs_dim) not in _FRESH:
        pol = S.policy(hidden, obs_dim)
        _FRESH[(hidden, obs_dim)] = S.sample_buffers(pol.flat, pol.spec, obs_dim, total=TOTAL, seed=11)
    return _FRESH[(hidden, obs_dim)]


def _call(k, dbuf, idx, n: int, K: int, *, mode: str = "minibatch", given=None, obs=None, **over):
    """one kp1_mlp_loss_grad into fresh outputs -> (grad [K, P], stats [K, 4]) on the device.  mode: "minibatch" (adv_inv_std = 0), "raw"
    (adv_inv_std < 0), "stats_dev" (given: [K, 2] device tensor), "scalars" (given: (mean, inv_std) passed as arguments)"""
    grad, stats = torch.full((K, k.num_params), NAN, device=DEV), torch.zeros((K, 4), device=DEV)
    kw = {**T.LOSS, **over}
    if mode == "scalars":
        o = dbuf["obs"] if obs is None else obs
        native.check(k.L.kp1_mlp_loss_grad(k._h, _p(o), o.shape[-1], _p(idx), n, _p(dbuf["act"]), _p(dbuf["old_logp"]), _p(dbuf["adv"]), _p(dbuf["ret"]),
                                           float(given[0]), float(given[1]), None, kw["clip_range"], kw["ent_coef"], kw["vf_coef"], 1.0 / n, _p(grad),
                                           _p(stats), 0, k._stream()))
    else:
        extra = {"normalize": False} if mode == "raw" else ({"adv_stats": given} if mode == "stats_dev" else {})
        S.loss_grad(k, dbuf, idx, n, grad, stats, obs=obs, **kw, **extra)
    return grad, stats


def _both(k, dbuf, idx, n: int, K: int, **kw):
    """layer-wise, then the tile twice (equal bits) -> ((grad, stats) layer-wise, (grad, stats) tile), on the CPU"""
    k.set_train_tile(False)
    lay = _call(k, dbuf, idx, n, K, **kw)
    k.set_train_tile(True)
    t1 = _call(k, dbuf, idx, n, K, **kw)
    t2 = _call(k, dbuf, idx, n, K, **kw)
    k.set_train_tile(False)
    torch.cuda.synchronize()
    assert k.train_tile is False
    assert torch.equal(t1[0].view(torch.int32), t2[0].view(torch.int32)) and torch.equal(t1[1].view(torch.int32), t2[1].view(torch.int32)), "two runs differ"
    return (lay[0].cpu(), lay[1].cpu()), (t1[0].cpu(), t1[1].cpu())


def _assert_hpart_bits(lay, tile, spec, what) -> None:
    """stats_out and the hpart-sum tensors of one replica: equal bits on both paths"""
    assert torch.equal(lay[1].view(torch.int32), tile[1].view(torch.int32)), (what, "stats", lay[1].tolist(), tile[1].tolist())
    sl = S.slices_of(spec)
    for name in HPART:
        a, b = lay[0][sl[name]], tile[0][sl[name]]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, name, (a - b).abs().max().item())


def _ratios(grad, stats, ref, spec, e32=None, what=None) -> dict[str, float]:
    assert torch.isfinite(grad).all() and torch.isfinite(stats).all(), what
    got = {"grad": grad, "policy_loss": stats[0].item(), "value_loss": stats[1].item(), "entropy": stats[2].item()}
    return T.ratios(T.loss_errors(got, ref, spec), T.loss_tolerances(ref, spec), e32)


def _record(case: str, lay_rat: dict, tile_rat: dict) -> None:
    _RATIOS[case] = {"layer-wise": {k: round(v, 4) for k, v in lay_rat.items()}, "train tile": {k: round(v, 4) for k, v in tile_rat.items()}}
    wl, wt = max(lay_rat, key=lay_rat.get), max(tile_rat, key=tile_rat.get)
    print(f"{case}: worst error / bound layer-wise {lay_rat[wl]:.3f} ({wl}), train tile {tile_rat[wt]:.3f} ({wt})")


def _assert_within(rat: dict[str, float], what) -> None:
    bad = {k: v for k, v in rat.items() if not v <= 1.0}
    assert not bad, (what, bad)


def _trained_refs(pol, obs_dim, buf, sel, regime: str, mode: str):
    ref = T.loss_reference(pol.flat, pol.spec, obs_dim, buf, sel, adv_mode=mode)
    e32 = None
    if regime == "T8":
        e32 = T.loss_errors(T.loss_reference(pol.flat, pol.spec, obs_dim, buf, sel, adv_mode=mode, dtype=torch.float32), ref, pol.spec)
    return ref, e32


# ================================================================================================ a + b, K = 1, fresh policies
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_fresh_policy_against_layerwise_and_fp64(world, kind, n):
    """option 0 then 1 on one handle: stats and the hpart-sum tensors equal bits, every tensor within the tolerances of fp64 autograd.
    n = 96 runs with idx = NULL (rows 0 .. 95 of gathered buffers), n = 31 with the observations at pitch 56 / 80, the others at the
    padded pitch through a permuted idx with repeats; n = 1 takes raw advantages (the unbiased std of one row is undefined)."""
    hidden, obs_dim, _ = kind
    pol, buf = _fresh(hidden, obs_dim)
    k, dbuf = world[0](kind), world[1]((hidden, obs_dim, "fresh"), buf)
    k.pack(pol.flat.to(DEV))
    sel = _rows(n)
    mode = "raw" if n == 1 else "minibatch"
    idx, obs, use = sel.to(DEV), None, dbuf
    if n == 96:
        idx, use = None, {name: t[sel.to(DEV)].contiguous() for name, t in dbuf.items()}
    if n == 31:
        obs = dbuf["obs"][:, :obs_dim].contiguous()
    lay, tile = _both(k, use, idx, n, 1, mode=mode, obs=obs)
    what = (kind, n)
    _assert_hpart_bits((lay[0][0], lay[1][0]), (tile[0][0], tile[1][0]), pol.spec, what)
    ref = S.reference(pol.flat, pol.spec, obs_dim, buf, sel, adv_mode=mode, **T.LOSS)
    rl, rt = _ratios(lay[0][0], lay[1][0], ref, pol.spec, what=what), _ratios(tile[0][0], tile[1][0], ref, pol.spec, what=what)
    if n > 1:
        klb = R.approx_kl_bound(pol.flat, pol.spec, obs_dim, buf["obs"][sel], buf["act"][sel], buf["old_logp"][sel])
        rt["approx_kl"] = S.check_kl(tile[1][0][3].item(), klb, what)
    _record(f"fresh {KIND_IDS[KINDS.index(kind)]} n={n}", rl, rt)
    _assert_within(rt, what)


# ================================================================================================ b, K = 1, trained scale
@pytest.mark.parametrize("n", T.NS)
@pytest.mark.parametrize("regime", ("T4", "T8"))
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_trained_scale_against_fp64(world, kind, regime, n):
    hidden, obs_dim, _ = kind
    pol, buf = T.case(hidden, obs_dim, regime)
    k, dbuf = world[0](kind), world[1]((hidden, obs_dim, regime), buf)
    k.pack(pol.flat.to(DEV))
    sel = _rows(n)
    lay, tile = _both(k, dbuf, sel.to(DEV), n, 1)
    what = (kind, regime, n)
    _assert_hpart_bits((lay[0][0], lay[1][0]), (tile[0][0], tile[1][0]), pol.spec, what)
    ref, e32 = _trained_refs(pol, obs_dim, buf, sel, regime, "minibatch")
    rl, rt = _ratios(lay[0][0], lay[1][0], ref, pol.spec, e32, what), _ratios(tile[0][0], tile[1][0], ref, pol.spec, e32, what)
    _record(f"trained {KIND_IDS[KINDS.index(kind)]} {regime} n={n}", rl, rt)
    _assert_within(rt, what)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_saturated_first_layer(world, kind):
    """observations times 1e18, T4 policy, n = 33: every output finite, the W1 / b1 gradients of the units saturated in every row exactly
    0, the rest under the T4 rule"""
    hidden, obs_dim, _ = kind
    n = 33
    pol, buf = T.case(hidden, obs_dim, "T4", saturated=True)
    k, dbuf = world[0](kind), world[1]((hidden, obs_dim, "saturated"), buf)
    k.pack(pol.flat.to(DEV))
    sel = _rows(n)
    lay, tile = _both(k, dbuf, sel.to(DEV), n, 1)
    what = (kind, "saturated")
    ref, _ = _trained_refs(pol, obs_dim, buf, sel, "T4", "minibatch")
    rl, rt = _ratios(lay[0][0], lay[1][0], ref, pol.spec, what=what), _ratios(tile[0][0], tile[1][0], ref, pol.spec, what=what)
    _record(f"saturated {KIND_IDS[KINDS.index(kind)]} n={n}", rl, rt)
    _assert_within(rt, what)
    parts, sl = T.hidden_parts(pol.flat, pol.spec, obs_dim, buf["obs"][sel]), S.slices_of(pol.spec)
    for net in parts:
        dead = (1 - parts[net]["h1"] ** 2 == 0).all(dim=0)
        assert bool(dead.any())
        w1 = tile[0][0][sl[f"mlp_extractor.{net}.0.weight"]].view(hidden, obs_dim)
        b1 = tile[0][0][sl[f"mlp_extractor.{net}.0.bias"]]
        assert not w1[dead].any() and not b1[dead].any(), (kind, net)


# ================================================================================================ a + b, K = 3
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_population_against_layerwise_and_fp64(world, kind, n):
    """K = 3 with distinct policies (T4, T8, T4), buffers and selections per replica: every replica as in the K = 1 tests"""
    hidden, obs_dim, _ = kind
    K = T.POP_K
    pols, buf = T.population(hidden, obs_dim)
    k, dbuf = world[0](kind, K), world[1]((hidden, obs_dim, "population"), buf)
    k.pack(torch.stack([p.flat for p in pols]).to(DEV).contiguous())
    sels = [r * TOTAL + _rows(n, r) for r in range(K)]
    idx = torch.stack(sels).to(DEV).contiguous()
    mode = "raw" if n == 1 else "minibatch"
    lay, tile = _both(k, dbuf, idx, n, K, mode=mode)
    assert not torch.equal(tile[0][0], tile[0][2])
    for r in range(K):
        regime, what = T.POP_REGIMES[r], (kind, "replica", r, n)
        _assert_hpart_bits((lay[0][r], lay[1][r]), (tile[0][r], tile[1][r]), pols[r].spec, what)
        ref, e32 = _trained_refs(pols[r], obs_dim, buf, sels[r], regime, mode)
        rl, rt = _ratios(lay[0][r], lay[1][r], ref, pols[r].spec, e32, what), _ratios(tile[0][r], tile[1][r], ref, pols[r].spec, e32, what)
        _record(f"population {KIND_IDS[KINDS.index(kind)]} replica {r} {regime} n={n}", rl, rt)
        _assert_within(rt, what)


# ================================================================================================ c: the advantage modes
@pytest.mark.parametrize("mode", ("minibatch", "stats_dev", "scalars"))
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_advantage_modes(world, kind, mode):
    """n = 33: statistics of the minibatch (adv_partials_kernel in front), adv_stats_dev, and the scalar arguments; the given statistics
    are not the minibatch's own, so a path that ignored them shows"""
    hidden, obs_dim, _ = kind
    n = 33
    pol, buf = _fresh(hidden, obs_dim)
    k, dbuf = world[0](kind), world[1]((hidden, obs_dim, "fresh"), buf)
    k.pack(pol.flat.to(DEV))
    sel = _rows(n)
    stats = (0.25, 0.5)
    given = None if mode == "minibatch" else (torch.tensor([stats], device=DEV) if mode == "stats_dev" else stats)
    lay, tile = _both(k, dbuf, sel.to(DEV), n, 1, mode=mode, given=given)
    what = (kind, mode)
    _assert_hpart_bits((lay[0][0], lay[1][0]), (tile[0][0], tile[1][0]), pol.spec, what)
    ref = S.reference(pol.flat, pol.spec, obs_dim, buf, sel, adv_mode="minibatch" if mode == "minibatch" else "given", adv_stats=stats, **T.LOSS)
    rt = _ratios(tile[0][0], tile[1][0], ref, pol.spec, what=what)
    _assert_within(rt, what)


# ================================================================================================ d: the per-replica table
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_replica_table_matches_single_handles(world, kind):
    """K = 3, distinct clip_range / vf_coef / ent_coef per replica: replica r equals, bit for bit, a K = 1 handle with the option on called
    with entry r's scalars (the chunking is a function of n alone)"""
    hidden, obs_dim, _ = kind
    K, n = T.POP_K, 96 + 33
    pols, buf = T.population(hidden, obs_dim)
    kp, k1 = world[0](kind, K), world[0](kind)
    dbuf = world[1]((hidden, obs_dim, "population"), buf)
    table = [dict(learning_rate=1e-3, adam_eps=1e-5, max_grad_norm=0.5, clip_range=0.1 + 0.05 * r, ent_coef=1e-3 * (r + 1), vf_coef=0.25 * (r + 1)) for r in range(K)]
    sels = [r * TOTAL + _rows(n, r) for r in range(K)]
    kp.pack(torch.stack([p.flat for p in pols]).to(DEV).contiguous())
    kp.set_replica_hparams(table)
    kp.set_train_tile(True)
    try:
        gp, sp = _call(kp, dbuf, torch.stack(sels).to(DEV).contiguous(), n, K, clip_range=9.0, ent_coef=9.0, vf_coef=9.0)   # the scalars are not read
    finally:
        kp.set_replica_hparams(None)
        kp.set_train_tile(False)
    k1.set_train_tile(True)
    for r in range(K):
        k1.pack(pols[r].flat.to(DEV))
        over = {f: table[r][f] for f in ("clip_range", "ent_coef", "vf_coef")}
        g1, s1 = _call(k1, dbuf, sels[r].to(DEV), n, 1, **over)
        torch.cuda.synchronize()
        assert torch.equal(gp[r].view(torch.int32), g1[0].view(torch.int32)), (kind, r, (gp[r] - g1[0]).abs().max().item())
        assert torch.equal(sp[r].view(torch.int32), s1[0].view(torch.int32)), (kind, r)
    k1.set_train_tile(False)
    assert not torch.equal(gp[0], gp[1])


# ================================================================================================ e: row attribution
@pytest.mark.parametrize("side", ("policy", "value"))
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_one_row_of_the_ragged_tile(world, kind, side):
    """n = 70 (tiles of 32, 32, 6): one row of the last tile carries loss, every other selected row contributes exactly nothing (policy
    side: advantage 0 with vf_coef = 0; value side: advantage 0 everywhere and the return = the handle's own value), rows outside the
    selection -- the positions >= n of a longer idx among them -- keep loud values.  inv_count = 1 / n, so the gradient is that row's fp64
    gradient / n; the tensors of the other side come out exactly 0."""
    hidden, obs_dim, _ = kind
    n, spike = 70, 67
    pol, buf = _fresh(hidden, obs_dim)
    k = world[0](kind)
    k.pack(pol.flat.to(DEV))
    long_idx = S.selection(TOTAL, n + 31, 4242)          # positions n .. n + 30 exist in the buffer and are not part of the minibatch
    sel = long_idx[:n]
    row = sel[spike:spike + 1]
    quiet = torch.ones(TOTAL, dtype=torch.bool)
    quiet[:] = False
    quiet[sel] = True
    quiet[row] = False
    b = {name: t.clone() for name, t in buf.items()}
    if side == "policy":
        b["adv"] = torch.where(quiet, torch.zeros_like(b["adv"]), b["adv"].abs() + 1.0)
        vf = 0.0
    else:
        own = torch.full((TOTAL,), NAN, device=DEV)
        k.forward(buf["obs"].to(DEV), value=own)
        torch.cuda.synchronize()
        b["adv"] = torch.zeros_like(b["adv"])
        b["ret"] = torch.where(quiet, own.cpu(), b["ret"] + 1.5)
        vf = 0.5
    db = S.dev(b)
    k.set_train_tile(True)
    grad, stats = _call(k, db, long_idx.to(DEV), n, 1, mode="raw", clip_range=R.CLIP_RANGE, ent_coef=0.0, vf_coef=vf)
    k.set_train_tile(False)
    torch.cuda.synchronize()
    grad = grad[0].cpu()
    ref = S.reference(pol.flat, pol.spec, obs_dim, b, row, clip_range=R.CLIP_RANGE, ent_coef=0.0, vf_coef=vf, adv_mode="raw")
    ref_grad = ref["grad"] / n
    rat = R.grad_errors(grad, ref_grad, pol.spec)
    reached = R.active(side)
    for name, sl in S.slices_of(pol.spec).items():
        if reached(name):
            assert ref_grad[sl].abs().max().item() > 0 and rat[name] <= 1.0, (kind, side, name, rat[name])
        else:
            assert not grad[sl].any(), (kind, side, name, grad[sl].abs().max().item())


# ================================================================================================ f: sequencing
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_four_adam_steps_and_a_graph_replay(kind):
    """S.ADAM's four loss_grad -> adam_step(flags 2, device step count) pairs (n = 200, 33, 200, 1) with the option on: p, m, v within
    S.adam_bounds of the fp64 restatement at every step, which at c0 = 0 also pins the device count (an off-by-one count violates the bound
    on every weight tensor).  Then one pair captured into a hipGraph and replayed from the same state: equal bits."""
    hidden, obs_dim, _ = kind
    a = S.ADAM
    pol = S.policy(hidden, obs_dim)
    buf = S.dev(S.sample_buffers(pol.flat, pol.spec, obs_dim, seed=a["seed"]))
    over = dict(clip_range=a["clip_range"], ent_coef=a["ent_coef"], vf_coef=a["vf_coef"])
    kw = dict(lr=a["lr"], eps=a["eps"], max_grad_norm=a["max_grad_norm"])
    k = S.handle(kind)
    k.set_train_tile(True)
    flat = pol.flat.to(DEV)
    k.pack(flat)
    k.set_step_count(0)
    p, m, v = flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)
    grads, states = [], []
    for i, n in enumerate(a["ns"]):
        idx = S.selection(S.TOTAL, n, 90 + i).to(DEV)
        grad, stats = torch.full((k.num_params,), NAN, device=DEV), torch.zeros(4, device=DEV)
        S.loss_grad(k, buf, idx, n, grad, stats, **({"normalize": False} if n == 1 else {}), **over)
        k.adam_step(p, grad, m, v, step=0, fused_norm=True, **kw)
        torch.cuda.synchronize()
        grads.append(grad.cpu())
        states.append((p.cpu(), m.cpu(), v.cpu()))
    assert all(torch.isfinite(g).all() for g in grads)
    ref64 = S.adam_restatement(pol.flat, grads, c0=0, dtype=torch.float64, **kw)
    ref32 = S.adam_restatement(pol.flat, grads, c0=0, dtype=torch.float32, **kw)
    bounds, errs = S.adam_bounds(ref64, ref32, pol.spec), S.adam_errors(ref64, states, pol.spec)
    bad = [(s, name, what, errs[s][name][what], bounds[s][name][what][1]) for s in range(len(errs)) for name, _ in pol.spec for what in "pmv"
           if not errs[s][name][what] <= bounds[s][name][what][1]]
    assert not bad, bad

    # one pair, eager and replayed, from the same state
    n = 200
    idx = S.selection(S.TOTAL, n, 90).to(DEV)
    grad, stats = torch.full((k.num_params,), NAN, device=DEV), torch.zeros(4, device=DEV)

    def pair():
        S.loss_grad(k, buf, idx, n, grad, stats, **over)
        k.adam_step(p, grad, m, v, step=0, fused_norm=True, **kw)

    def start():
        p.copy_(flat), m.zero_(), v.zero_(), stats.zero_(), grad.fill_(NAN)
        k.pack(p)
        k.set_step_count(0)
        torch.cuda.synchronize()

    start()
    pair()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (p, m, v, grad, stats)]
    start()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pair()
    start()
    g.replay()
    torch.cuda.synchronize()
    for name, x, y in zip(("p", "m", "v", "grad", "stats"), eager, (p, m, v, grad, stats)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (kind, name)
    assert not torch.equal(p, flat)
    k.close()


# ================================================================================================ g: fallback and refusal
def test_more_rows_than_the_slabs_cover_take_the_layerwise_launches():
    """max_batch = 4096, n = 2049 (65 tiles > 64 slabs): the gradient with the option on is the option-off gradient, bit for bit"""
    kind = KINDS[0]
    hidden, obs_dim, _ = kind
    n = 2049
    pol = S.policy(hidden, obs_dim)
    buf = S.sample_buffers(pol.flat, pol.spec, obs_dim, total=2304, seed=12)
    dbuf = S.dev(buf)
    k = S.handle(kind, max_batch=4096)
    k.pack(pol.flat.to(DEV))
    idx = S.selection(2304, n, 77).to(DEV)
    lay, tile = _both(k, dbuf, idx, n, 1)
    k.close()
    assert torch.isfinite(lay[0]).all()
    assert torch.equal(lay[0].view(torch.int32), tile[0].view(torch.int32)) and torch.equal(lay[1].view(torch.int32), tile[1].view(torch.int32))


def test_hidden_256_refuses_the_option():
    kind = S.KINDS[0]
    hidden, obs_dim, _ = kind
    pol = S.policy(hidden, obs_dim)
    buf = S.dev(S.sample_buffers(pol.flat, pol.spec, obs_dim, seed=11))
    k = S.handle(kind)
    k.pack(pol.flat.to(DEV))
    idx, n = S.selection(S.TOTAL, 33, 5).to(DEV), 33
    before = _call(k, buf, idx, n, 1)
    rc = k.L.kp1_mlp_set_option(k._h, 6, 1)
    assert rc == KP1_ERR_UNSUPPORTED
    text = native.load().kp1_last_error().decode()
    assert "KP1_MLP_OPT_TRAIN_TILE" in text and "256" in text, text
    with pytest.raises(native.Kp1Error, match="KP1_MLP_OPT_TRAIN_TILE"):
        k.set_train_tile(True)
    assert k.train_tile is False
    after = _call(k, buf, idx, n, 1)
    torch.cuda.synchronize()
    assert torch.equal(before[0].view(torch.int32), after[0].view(torch.int32)) and torch.equal(before[1].view(torch.int32), after[1].view(torch.int32))
    k.close()


# ================================================================================================ h: the trainers
def _approach_cfg():
    from rl_brain_trainer_amd import config as kcfg

    return kcfg.to_env_config(kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"))


def _first_step_sums(trainer) -> list:
    """wraps the handle's loss_grad: the loss sums after the first optimiser step of the next train() (its first epoch runs eagerly)"""
    first, orig = [], trainer._mlp.loss_grad

    def wrapped(*args, **kw):
        orig(*args, **kw)
        if not first:
            first.append(kw["stats_out"].clone())

    trainer._mlp.loss_grad = wrapped
    return first


def _train(make, form: str, monkeypatch):
    monkeypatch.setenv("KP1_TRAIN_TILE", form)
    trainer, closers = make()
    assert trainer._mlp.train_tile is (form == "1")
    trainer.collect_rollouts()
    first = _first_step_sums(trainer)
    trainer.train()                       # two epochs: one eager, one captured and replayed
    torch.cuda.synchronize()
    out = dict(first=first[0].cpu(), flat=trainer.flat.detach().cpu().clone(), form=trainer.update_form, key=trainer._epoch_key(),
               graph=trainer._epoch_graph is not None, replica_form=trainer.replica(0).update_form if hasattr(trainer, "replica") else None)
    trainer._mlp.close()
    for c in closers:
        c.close()
    return out


def _compare_forms(make, monkeypatch):
    on, off = _train(make, "1", monkeypatch), _train(make, "0", monkeypatch)
    assert on["graph"] and off["graph"]
    assert torch.equal(on["first"].view(torch.int32), off["first"].view(torch.int32)), (on["first"].tolist(), off["first"].tolist())
    assert bool(on["first"][:, :2].abs().min() > 0)
    assert torch.isfinite(on["flat"]).all() and torch.isfinite(off["flat"]).all()
    assert on["form"].startswith("train tile") and off["form"] == "layer-wise"
    assert on["key"] != off["key"]
    return on, off


def test_ppo_trains_with_the_tile(monkeypatch):
    from rl_brain_trainer_amd.ppo import PPO, PPOConfig
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    def make():
        env = ArmKinematicVecEnv(_approach_cfg(), 16, seed=21)
        return PPO(env, PPOConfig(n_steps=64, batch_size=256, n_epochs=2, hidden=64, learning_rate=3e-4, seed=5)), [env]

    _compare_forms(make, monkeypatch)


def test_approach_population_trains_with_the_tile(monkeypatch):
    from rl_brain_trainer_amd.population import ApproachPopulationPPO
    from rl_brain_trainer_amd.ppo import PPOConfig
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    def make():
        seeds = [7, 8]
        env = ArmKinematicPopulationVecEnv(_approach_cfg(), seeds, 16)
        return ApproachPopulationPPO(seeds, PPOConfig(n_steps=64, batch_size=256, n_epochs=2, hidden=64, learning_rate=3e-4, ent_coef=1e-3), env), [env]

    on, _ = _compare_forms(make, monkeypatch)
    assert on["replica_form"].startswith("train tile")
