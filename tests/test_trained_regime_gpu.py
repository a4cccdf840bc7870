"""The MLP kernels on trained-scale policies against fp64 (tests/trained_regime.py: regimes T4 and T8, observation entries on the clip bound,
sigma of 0.01 .. 0.1).  Every older comparison of these kernels with an outside reference runs on a freshly initialised policy, where no
hidden unit passes |h| = 0.999; here 40 % (T4) to 70 % (T8) of the second-layer units do, pre-activations reach 20 .. 49, and one case
drives every first-layer unit to exactly +-1.

  forward    mean, value, action, clipped and log_prob (from the supplied noise) of the selected rows against fp64
  loss_grad  minibatch-normalised advantages, clip_range 0.1, ent_coef 1e-3, vf_coef 0.5 (and one raw-advantage case on the fused and the
             2x64 kinds): the gradient per tensor, the three losses, approx_kl under R.approx_kl_bound; two runs give equal bits
  kinds      the five of S.KINDS and the K = 3 populations of S.POP_KINDS (own seed per replica; regimes T4, T8, T4)
  rows       gathered from a 1024-row buffer.  n = 33: a one-row second tile.  n = 520: past 512; R.units gives the partitions -- fused
             path 17 row tiles of 32 (the last with 8 rows), five dW2 chunks of 128 rows and nine dW1 chunks of 64, the last of each holding
             8 rows; layer-wise path nine 64-row tiles / chunks, the last ragged
  bounds     T4: the project's existing tolerances, unchanged (the CPU companion shows a float32 evaluation uses <= 0.1 of each there).
             T8: max(existing tolerance, 8 e32) per tensor or output, e32 = |float32 torch on the CPU - fp64| on the same rows

test_trained_regime_cpu.py asserts the conditions that give these checks their power.  Every check prints error / bound; one MI355X run of
them: profiles/trained_regime_parity.json."""
from __future__ import annotations

import json
import os

import pytest
import torch

import mlp_handle_state as S
import row_attribution as R
import trained_regime as T

pytestmark = pytest.mark.gpu
DEV = S.DEV
NAN = float("nan")
MAX_BATCH = 1024
FWD = {"mean": 7, "value": 0, "action": 7, "clipped": 7, "log_prob": 0}
_WORST: dict[str, dict[str, float]] = {}      # case -> check -> error / bound, what the last run measured


@pytest.fixture(scope="module")
def world():
    """per (kind, K): one handle, reused by every case of the kind (as training reuses it); per net and regime: the buffers on the device.
    KP1_TRAINED_REGIME_OUT=<file>: the measured error / bound ratios are written there when the module is done."""
    handles, bufs = {}, {}

    def get_handle(kind, K=1):
        if (kind, K) not in handles:
            handles[(kind, K)] = S.handle(kind, max_batch=MAX_BATCH, replicas=K)
        return handles[(kind, K)]

    def get_buf(key, buf):
        if key not in bufs:
            bufs[key] = S.dev(buf)
        return bufs[key]

    yield get_handle, get_buf
    for k in handles.values():
        k.close()
    out = os.environ.get("KP1_TRAINED_REGIME_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(_WORST, f, indent=1, sort_keys=True)


def _record(case: str, rat: dict[str, float]) -> None:
    _WORST.setdefault(case, {}).update({k: round(v, 4) for k, v in rat.items()})
    worst = max(rat, key=rat.get)
    print(f"{case}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in rat.items()) + f" -- worst {rat[worst]:.3f} ({worst})")


def _forward(k, dbuf, idx) -> dict[str, torch.Tensor]:
    rows = idx.numel()
    out = {name: torch.full((rows, w) if w else (rows,), NAN, device=DEV) for name, w in FWD.items()}
    k.forward(dbuf["obs"][idx].contiguous(), noise=dbuf["noise"][idx].contiguous(), **out)
    return out


def _loss_grad_twice(k, dbuf, idx, n: int, K: int, **over):
    """two runs into fresh outputs: equal bits (the kernels' reductions have a fixed order) -> grad [K, P], stats [K, 4]"""
    runs = []
    for _ in range(2):
        grad, stats = torch.full((K, k.num_params), NAN, device=DEV), torch.zeros((K, 4), device=DEV)
        S.loss_grad(k, dbuf, idx, n, grad, stats, **{**T.LOSS, **over})
        runs.append((grad, stats))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    return runs[0][0].cpu(), runs[0][1].cpu()


def _forward_ratios(got: dict, pol, obs_dim: int, buf: dict, sel, regime: str) -> dict[str, float]:
    ref = T.forward_reference(pol.flat, pol.spec, obs_dim, buf["obs"][sel], buf["noise"][sel])
    e32 = None
    if regime == "T8":
        e32 = T.forward_errors(T.forward_reference(pol.flat, pol.spec, obs_dim, buf["obs"][sel], buf["noise"][sel], dtype=torch.float32), ref)
    assert all(torch.isfinite(t).all() for t in got.values())
    return T.forward_ratios(got, ref, e32)


def _loss_ratios(grad, stats, pol, obs_dim: int, buf: dict, sel, regime: str, mode: str, what) -> dict[str, float]:
    ref = T.loss_reference(pol.flat, pol.spec, obs_dim, buf, sel, adv_mode=mode)
    e32 = None
    if regime == "T8":
        e32 = T.loss_errors(T.loss_reference(pol.flat, pol.spec, obs_dim, buf, sel, adv_mode=mode, dtype=torch.float32), ref, pol.spec)
    assert torch.isfinite(grad).all() and torch.isfinite(stats).all(), what
    got = {"grad": grad, "policy_loss": stats[0].item(), "value_loss": stats[1].item(), "entropy": stats[2].item()}
    rat = T.ratios(T.loss_errors(got, ref, pol.spec), T.loss_tolerances(ref, pol.spec), e32)
    klb = R.approx_kl_bound(pol.flat, pol.spec, obs_dim, buf["obs"][sel], buf["act"][sel], buf["old_logp"][sel])
    assert abs(klb["kl64"] - ref["approx_kl"]) <= 1e-12 * abs(ref["approx_kl"]), what
    rat["approx_kl"] = S.check_kl(stats[3].item(), klb, what)
    return rat


def _assert_within(rat: dict[str, float], what) -> None:
    bad = {k: v for k, v in rat.items() if not v <= 1.0}
    assert not bad, (what, bad)


# ================================================================================================ K = 1
GRID = [(kd, regime, n) for kd in S.KINDS for regime in T.REGIMES for n in T.NS]
GRID_IDS = [f"{S.KIND_IDS[S.KINDS.index(kd)]}-{regime}-n{n}" for kd, regime, n in GRID]
LOSS_GRID = [(kd, regime, n, "minibatch") for kd, regime, n in GRID] + [(kd, "T4", 520, "raw") for kd in S.KINDS if kd[2] == "fused" or kd[0] == 64]
LOSS_IDS = [f"{S.KIND_IDS[S.KINDS.index(kd)]}-{regime}-n{n}-{mode}" for kd, regime, n, mode in LOSS_GRID]


@pytest.mark.parametrize("kind,regime,n", GRID, ids=GRID_IDS)
def test_forward_against_fp64(world, kind, regime, n):
    """rtol 1e-4 / atol 2e-5 for mean, value, action and clipped, 1e-4 / 1e-4 for log_prob; at T8 each widened to 8 e32 where that is larger"""
    hidden, obs_dim, _ = kind
    pol, buf = T.case(hidden, obs_dim, regime)
    k, dbuf = world[0](kind), world[1]((hidden, obs_dim, regime), buf)
    k.pack(pol.flat.to(DEV))
    sel = T.rows(n)
    got = _forward(k, dbuf, sel.to(DEV))
    rat = _forward_ratios(got, pol, obs_dim, buf, sel, regime)
    _record(f"forward {S.KIND_IDS[S.KINDS.index(kind)]} {regime} n={n}", rat)
    _assert_within(rat, (kind, regime, n))


@pytest.mark.parametrize("kind,regime,n,mode", LOSS_GRID, ids=LOSS_IDS)
def test_loss_grad_against_fp64(world, kind, regime, n, mode):
    """gradient per tensor 2e-4 max|ref| + 1e-7, losses 1e-4 (|x| + 1), entropy 1e-5; at T8 each widened to 8 e32 where that is larger;
    approx_kl under S.check_kl's bound in both regimes"""
    hidden, obs_dim, _ = kind
    pol, buf = T.case(hidden, obs_dim, regime)
    k, dbuf = world[0](kind), world[1]((hidden, obs_dim, regime), buf)
    k.pack(pol.flat.to(DEV))
    sel = T.rows(n)
    grad, stats = _loss_grad_twice(k, dbuf, sel.to(DEV), n, 1, **({"normalize": False} if mode == "raw" else {}))
    what = (kind, regime, n, mode)
    rat = _loss_ratios(grad[0], stats[0], pol, obs_dim, buf, sel, regime, mode, what)
    _record(f"loss_grad {S.KIND_IDS[S.KINDS.index(kind)]} {regime} n={n} {mode}", rat)
    _assert_within(rat, what)


# ================================================================================================ K = 3
@pytest.mark.parametrize("n", T.NS)
@pytest.mark.parametrize("hidden,obs_dim", S.POP_KINDS)
def test_population_against_fp64(world, hidden, obs_dim, n):
    """one population handle, replica r with its own policy (regimes T4, T8, T4), its own 1024 buffer rows and its own selection: forward
    and loss_grad of every replica against its own fp64 reference, each under its own regime's bounds"""
    kind, K = (hidden, obs_dim, "layer"), T.POP_K
    pols, buf = T.population(hidden, obs_dim)
    k, dbuf = world[0](kind, K), world[1]((hidden, obs_dim, "population"), buf)
    k.pack(torch.stack([p.flat for p in pols]).to(DEV).contiguous())
    sels = [r * T.TOTAL + T.rows(n, r) for r in range(K)]
    idx = torch.stack(sels).to(DEV).contiguous()
    fwd = _forward(k, dbuf, idx.reshape(-1))
    grad, stats = _loss_grad_twice(k, dbuf, idx, n, K)
    assert not torch.equal(grad[0], grad[2])
    for r in range(K):
        regime, what = T.POP_REGIMES[r], (kind, "replica", r, n)
        rat = _forward_ratios({name: t[r * n:(r + 1) * n] for name, t in fwd.items()}, pols[r], obs_dim, buf, sels[r], regime)
        rat.update(_loss_ratios(grad[r], stats[r], pols[r], obs_dim, buf, sels[r], regime, "minibatch", what))
        _record(f"population {hidden}-{obs_dim} replica {r} {regime} n={n}", rat)
        _assert_within(rat, what)


# ================================================================================================ saturation
@pytest.mark.parametrize("kind", S.KINDS, ids=S.KIND_IDS)
def test_saturated_first_layer(world, kind):
    """T.saturated_buffers (observations times 1e18) at n = 33, T4 policy: every layer-1 pre-activation is ~ 1e18, so 2^(-2 log2(e) x) is 0
    or inf and kp_tanh must return exactly +-1.  Every forward output and every gradient element is finite; the forward outputs meet the
    forward tolerances; the W1 and b1 gradients of the units whose fp64 1 - h1^2 is exactly 0 in every selected row (all of them: CPU
    companion) are exactly 0; the other tensors and the losses meet the T4 rule."""
    hidden, obs_dim, _ = kind
    n = T.NS[0]
    pol, buf = T.case(hidden, obs_dim, "T4", saturated=True)
    k, dbuf = world[0](kind), world[1]((hidden, obs_dim, "saturated"), buf)
    k.pack(pol.flat.to(DEV))
    sel = T.rows(n)
    rat = _forward_ratios(_forward(k, dbuf, sel.to(DEV)), pol, obs_dim, buf, sel, "T4")
    grad, stats = _loss_grad_twice(k, dbuf, sel.to(DEV), n, 1)
    rat.update(_loss_ratios(grad[0], stats[0], pol, obs_dim, buf, sel, "T4", "minibatch", (kind, "saturated")))
    _record(f"saturated {S.KIND_IDS[S.KINDS.index(kind)]} n={n}", rat)
    _assert_within(rat, (kind, "saturated"))
    parts, sl = T.hidden_parts(pol.flat, pol.spec, obs_dim, buf["obs"][sel]), S.slices_of(pol.spec)
    for net in parts:
        dead = (1 - parts[net]["h1"] ** 2 == 0).all(dim=0)                              # [hidden]: units saturated in every selected row
        assert bool(dead.any())
        w1 = grad[0][sl[f"mlp_extractor.{net}.0.weight"]].view(hidden, obs_dim)
        b1 = grad[0][sl[f"mlp_extractor.{net}.0.bias"]]
        assert not w1[dead].any() and not b1[dead].any(), (kind, net, w1[dead].abs().max().item(), b1[dead].abs().max().item())
