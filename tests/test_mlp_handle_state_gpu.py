"""The training handle as training uses it: one MlpKernels handle reused across calls of different sizes, paths and options; the smallest
minibatches; the clip coefficient of both norm routes; and the device step count over several Adam steps.  Every other test of these
kernels makes one call on a fresh, zero-filled handle, and the population / graph tests compare the kernels with themselves.

  1. history independence (bitwise): a fixed probe gives the same bits on a fresh handle and after any history of other calls
  2. nothing outside the selection is read, nothing outside the outputs is written (bitwise)
  3. exp_avg after one step from m = 0 is fl(0.1f * fl(g * c)): the clip coefficient c of both norm routes against fp64
  4. four Adam steps on the device step count against an fp64 restatement fed the device's own gradients
  5. n = 1 .. 129 and the tile / chunk / kernel-shape switches against torch autograd in fp64

Inputs and references come from tests/mlp_handle_state.py (CPU); test_mlp_handle_state_cpu.py asserts the conditions that give 3 and 4 their
power.  Values of one MI355X run of 4: profiles/mlp_handle_state_parity.json."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import mlp_handle_state as S
import row_attribution as R
from rl_brain_trainer_amd import ppo as P
from rl_brain_trainer_amd.mlp import MlpKernels

pytestmark = pytest.mark.gpu
DEV, KW = S.DEV, S.KW
_handle, _dev, _loss_grad, _check_kl = S.handle, S.dev, S.loss_grad, S.check_kl      # the call helpers shared with test_trained_regime_gpu.py
ADAM_KW = dict(lr=3e-4, eps=1e-5, max_grad_norm=0.5)
NAN = float("nan")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


# ================================================================================================ 1. history independence
class _World:
    """One kind's fixed probe inputs and the material of the histories.  K > 1: a population handle, every per-net tensor with a leading
    replica axis."""

    def __init__(self, kind, K=1):
        hidden, obs_dim, _ = kind
        self.kind, self.K, self.D, self.W = kind, K, obs_dim, S.pitch(obs_dim)
        pols = [S.policy(hidden, obs_dim, seed=3 + 10 * r) for r in range(K)]
        others = [S.policy(hidden, obs_dim, seed=5 + 10 * r, head_scale=20.0) for r in range(K)]
        self.spec = pols[0].spec
        self.flat0 = torch.stack([p.flat for p in pols]).to(DEV).contiguous()          # [K][P]
        self.other = torch.stack([p.flat for p in others]).to(DEV).contiguous()
        self.buf = _dev(S.sample_buffers(pols[0].flat, self.spec, obs_dim, seed=1))
        self.idx33 = torch.stack([S.selection(S.TOTAL, 33, 100 + r) for r in range(K)]).to(DEV).contiguous()
        self.idx1 = torch.stack([S.selection(S.TOTAL, 1, 200 + r) for r in range(K)]).to(DEV).contiguous()
        g = torch.Generator(device="cpu").manual_seed(17)
        fobs = torch.zeros((K * 40, self.W))
        fobs[:, :obs_dim] = torch.rand((K * 40, obs_dim), generator=g) * 2 - 1
        self.fobs, self.fnoise = fobs.to(DEV), torch.randn((K * 40, 7), generator=g).to(DEV)
        # histories: a full-size call on other data
        self.big = _dev(S.sample_buffers(others[0].flat, self.spec, obs_dim, seed=2))
        self.big["adv"] = self.big["adv"] * 1e3
        self.big["ret"] = self.big["ret"] * 1e3
        self.big_idx = torch.stack([S.selection(S.TOTAL, 512, 300 + r) for r in range(K)]).to(DEV).contiguous()
        self.nan_obs = self.big["obs"].clone()
        self.nan_obs[:, :obs_dim] = NAN                                                 # pad columns stay zero
        hobs = torch.zeros((K * 512, self.W))
        hobs[:, :obs_dim] = (torch.rand((K * 512, obs_dim), generator=g) * 2 - 1) * 5.0
        self.hobs, self.hnoise = hobs.to(DEV), torch.randn((K * 512, 7), generator=g).to(DEV)
        self.teacher = torch.randn((S.TOTAL, 7), generator=g).to(DEV).contiguous()
        self.idx200 = torch.stack([S.selection(S.TOTAL, 200, 400 + r) for r in range(K)]).to(DEV).contiguous()

    def single(self, r: int) -> "_World":
        """replica r's share as a K = 1 world (same tensors, sliced)"""
        w = object.__new__(_World)
        w.__dict__.update(self.__dict__)
        w.K = 1
        w.flat0, w.idx33, w.idx1 = self.flat0[r:r + 1].contiguous(), self.idx33[r:r + 1].contiguous(), self.idx1[r:r + 1].contiguous()
        w.fobs, w.fnoise = self.fobs[40 * r:40 * (r + 1)].contiguous(), self.fnoise[40 * r:40 * (r + 1)].contiguous()
        return w


def _probe(k: MlpKernels, w: _World) -> dict[str, torch.Tensor]:
    K, Pn = w.K, k.num_params
    k.pack(w.flat0)
    k.set_step_count(0)
    k.set_actor_extra_steps(0)
    p, m, v = w.flat0.clone(), torch.zeros_like(w.flat0), torch.zeros_like(w.flat0)
    out = {}
    for n, idx in ((33, w.idx33), (1, w.idx1)):
        grad = torch.full((K, Pn), NAN, device=DEV)
        stats = torch.zeros((K, 4), device=DEV)
        _loss_grad(k, w.buf, idx, n, grad, stats)
        k.adam_step(p, grad, m, v, step=0, fused_norm=True, **ADAM_KW)
        out.update({f"grad{n}": grad, f"stats{n}": stats, f"p{n}": p.clone(), f"m{n}": m.clone(), f"v{n}": v.clone()})
        if n == 33:
            fw = {"mean": torch.full((K * 40, 7), NAN, device=DEV), "value": torch.full((K * 40,), NAN, device=DEV),
                  "action": torch.full((K * 40, 7), NAN, device=DEV), "log_prob": torch.full((K * 40,), NAN, device=DEV)}
            k.forward(w.fobs, noise=w.fnoise, **fw)
            out.update(fw)
    torch.cuda.synchronize()
    k.pack(w.flat0)          # the handle no longer refers to the scratch parameters
    return out


def _history(k: MlpKernels, w: _World, which: str) -> None:
    K, Pn, (hidden, _, path) = w.K, k.num_params, w.kind
    grad, stats = torch.empty((K, Pn), device=DEV), torch.zeros((K, 4), device=DEV)
    k.pack(w.other)
    if which in ("a", "e"):      # a full-size minibatch of large finite data (e: NaN in every selected observation row)
        _loss_grad(k, w.big, w.big_idx, 512, grad, stats, obs=w.nan_obs if which == "e" else None)
        assert torch.isnan(grad).any() if which == "e" else (K > 1 or torch.isfinite(grad).all())
    elif which == "b":           # a full-size forward pass
        outs = {"mean": torch.empty((K * 512, 7), device=DEV), "value": torch.empty(K * 512, device=DEV), "action": torch.empty((K * 512, 7), device=DEV),
                "clipped": torch.empty((K * 512, 7), device=DEV), "log_prob": torch.empty(K * 512, device=DEV)}
        k.forward(w.hobs, noise=w.hnoise, **outs)
    elif which == "c_path":      # the other path of the 256-wide handle, over the same workspace
        k.set_fused(path != "fused")
        _loss_grad(k, w.big, w.big_idx, 300, grad, stats)
        k.set_fused(path == "fused")
    elif which == "c_bf16x3":    # the bf16x3 weight-gradient planes and slabs
        k.set_bf16x3_wgrad(True)
        _loss_grad(k, w.big, w.big_idx, 300, grad, stats)
        k.set_bf16x3_wgrad(False)
    elif which == "d":           # the teacher-anchor side step (raises the actor-extra count)
        loss = torch.empty(K, device=DEV)
        p, m, v = w.other.clone(), torch.zeros_like(w.other), torch.zeros_like(w.other)
        k.anchor_loss_grad(w.big["obs"], w.idx200, 200, w.teacher, loss_weight=0.5, grad_out=grad, loss_out=loss)
        k.anchor_adam_step(p, grad, m, v, step=0, **ADAM_KW)
        torch.cuda.synchronize()
        k.pack(w.other)
    else:
        raise AssertionError(which)
    torch.cuda.synchronize()


def _histories(kind) -> list[str]:
    hidden, _, path = kind
    h = ["a", "b"]
    if hidden == 256:
        h.append("c_path")
        if path == "fused":
            h.append("c_bf16x3")
    else:
        h.append("d")
    return h + ["e"]


def _assert_same(got: dict, want: dict, what) -> None:
    bad = [name for name in want if not torch.equal(got[name], want[name])]
    assert not bad, (what, bad, {name: int((_bits(got[name]) != _bits(want[name])).sum()) for name in bad})


@pytest.mark.parametrize("kind", S.KINDS, ids=S.KIND_IDS)
def test_probe_is_independent_of_the_handles_history(kind):
    """The probe (loss_grad + adam_step at n = 33, a 40-row forward, loss_grad + adam_step at n = 1; every output, bit for bit) on a handle
    that has been through each history in turn equals the probe on a fresh, zero-filled handle.  Between history and probe only the declared
    state is restored, through the API: the packed weights, the step count, the actor-extra count and the options.  History e leaves NaN
    in every activation, slab and partial it writes, so a stale value that the probe reads and 'multiplies by zero' comes out as NaN."""
    w = _World(kind)
    fresh = _handle(kind)
    want = _probe(fresh, w)
    fresh.close()
    assert all(torch.isfinite(t).all() for t in want.values())
    assert (want["p33"] != w.flat0).any() and (want["p1"] != want["p33"]).any() and not torch.equal(want["grad1"], want["grad33"])
    k = _handle(kind)
    for which in _histories(kind):
        _history(k, w, which)
        _assert_same(_probe(k, w), want, which)
    k.close()


@pytest.mark.parametrize("hidden,obs_dim", S.POP_KINDS)
def test_population_probe_is_independent_of_history_and_matches_single_handles(hidden, obs_dim):
    """K = 3 population handle through histories a, b and e; and replica k's probe equals the probe of a K = 1 layer-wise handle holding
    replica k's weights (test_population_kernels_match_single_handles asserts that of fresh handles only)."""
    kind, K = (hidden, obs_dim, "layer"), 3
    w = _World(kind, K)
    fresh = _handle(kind, replicas=K)
    want = _probe(fresh, w)
    fresh.close()
    assert all(torch.isfinite(t).all() for t in want.values())
    # stats_out [K][4]: each replica's approx_kl against its own fp64 reference (its own policy on its own rows); the K references differ
    cpu, kls = {name: t.cpu() for name, t in w.buf.items()}, []
    for r in range(K):
        sel = w.idx33[r].cpu()
        klb = R.approx_kl_bound(w.flat0[r], w.spec, obs_dim, cpu["obs"][sel], cpu["act"][sel], cpu["old_logp"][sel])
        ref = S.reference(w.flat0[r], w.spec, obs_dim, cpu, sel, adv_mode="minibatch", **KW)
        assert abs(klb["kl64"] - ref["approx_kl"]) <= 1e-12 * ref["approx_kl"]
        ratio = _check_kl(want["stats33"][r, 3].item(), klb, (kind, "replica", r))
        print(f"{kind} replica {r}: approx_kl {want['stats33'][r, 3].item():.6e} error / bound {ratio:.3f}")
        kls.append(klb)
    assert all(abs(kls[a]["kl64"] - kls[b]["kl64"]) > kls[a]["bound"] + kls[b]["bound"] for a in range(K) for b in range(a + 1, K))
    k = _handle(kind, replicas=K)
    for which in ("a", "b", "e"):
        _history(k, w, which)
        _assert_same(_probe(k, w), want, which)
    k.close()
    for r in range(K):
        s = _handle(kind)
        one = _probe(s, w.single(r))
        s.close()
        for name, t in want.items():
            rows = t.shape[0] // K
            assert torch.equal(one[name].reshape(t[rows * r:rows * (r + 1)].shape), t[rows * r:rows * (r + 1)]), (name, r)
    assert not torch.equal(want["p33"][0], want["p33"][1])


# ================================================================================================ 2. reads and writes stay inside
SENTINEL = 0x7FC5A5A5      # a quiet NaN with a payload no kernel produces
GUARD = 256


def _guarded(numel: int, fill: float = NAN) -> torch.Tensor:
    t = torch.empty(numel + GUARD, device=DEV)
    t[:numel] = fill
    t[numel:].view(torch.int32).fill_(SENTINEL)
    return t


def _guard_intact(t: torch.Tensor, numel: int) -> bool:
    return bool((t[numel:].view(torch.int32) == SENTINEL).all())


def _poisoned(buf: dict, keep_rows: torch.Tensor, obs_dim: int) -> dict:
    """NaN in every row that is not in keep_rows (pad columns of obs excepted: the kernels read them and they must be zero)"""
    out = {}
    drop = torch.ones(buf["obs"].shape[0], dtype=torch.bool, device=DEV)
    drop[keep_rows] = False
    for name in ("obs", "act", "old_logp", "adv", "ret"):
        t = buf[name].clone()
        if name == "obs":
            t[drop, :obs_dim] = NAN
        else:
            t[drop] = NAN
        out[name] = t
    return out


# population handles gather through idx only (kp1_mlp_loss_grad rejects idx = NULL for them)
READ_CASES = [(kd, 1, n, gather) for kd in S.KINDS for n in (1, 33) for gather in (True, False)] + [((64, 56, "layer"), 3, n, True) for n in (1, 33)]


@pytest.mark.parametrize("kind,K,n,gather", READ_CASES,
                         ids=[f"{kd[0]}-{kd[1]}-{kd[2]}-K{K}-n{n}-{'idx' if gather else 'prefix'}" for kd, K, n, gather in READ_CASES])
def test_loss_grad_touches_only_its_selection_and_its_outputs(kind, K, n, gather):
    """Two runs, equal bits: clean buffers, and NaN in every row of obs, actions, old_logp, adv and ret that the call does not select (rows
    >= n without idx), the unused tail of an over-long idx pointing at such a row.  grad_out (started from NaN) and stats_out are the heads
    of larger tensors whose 256-float tails hold a sentinel: every legitimate element is overwritten, the tails are untouched."""
    hidden, obs_dim, _ = kind
    pols = [S.policy(hidden, obs_dim, seed=3 + 10 * r) for r in range(K)]
    flat = torch.stack([p.flat for p in pols]).to(DEV).contiguous()
    buf = _dev(S.sample_buffers(pols[0].flat, pols[0].spec, obs_dim, seed=4))
    k = _handle(kind, replicas=K)
    k.pack(flat)
    Pn = k.num_params
    if gather:   # an over-long index tensor: entries past the K * n that are used point at the last row
        idx_buf = torch.full((K * n + 64,), S.TOTAL - 1, dtype=torch.int64, device=DEV)
        sel = torch.stack([S.selection(S.TOTAL - 1, n, 500 + r) for r in range(K)]).to(DEV)       # never the last row
        idx_buf[:K * n] = sel.reshape(-1)
        idx, rows = idx_buf[:K * n], sel.reshape(-1)
    else:
        idx, rows = None, torch.arange(n, device=DEV)
    runs = []
    for b in (buf, _poisoned(buf, rows, obs_dim)):
        grad, stats = _guarded(K * Pn), _guarded(K * 4, fill=0.0)
        _loss_grad(k, b, idx, n, grad[:K * Pn], stats[:K * 4])
        torch.cuda.synchronize()
        assert _guard_intact(grad, K * Pn) and _guard_intact(stats, K * 4)
        assert torch.isfinite(grad[:K * Pn]).all() and torch.isfinite(stats[:K * 4]).all()     # every element overwritten, nothing poisoned read
        runs.append((grad[:K * Pn].clone(), stats[:K * 4].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert (runs[0][0] != 0).any()
    k.close()


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("kind,K", [(kd, 1) for kd in S.KINDS] + [((64, 56, "layer"), 3)], ids=S.KIND_IDS + ["64-56-K3"])
def test_forward_touches_only_its_rows_and_its_outputs(kind, K, n):
    """forward over the first K * n rows of longer obs / noise buffers, clean and with NaN tails: equal bits; each of the five outputs is the
    head of a larger tensor whose sentinel tail stays untouched."""
    hidden, obs_dim, _ = kind
    W = S.pitch(obs_dim)
    pols = [S.policy(hidden, obs_dim, seed=3 + 10 * r) for r in range(K)]
    k = _handle(kind, replicas=K)
    k.pack(torch.stack([p.flat for p in pols]).to(DEV).contiguous())
    g = torch.Generator(device="cpu").manual_seed(23)
    rows, extra = K * n, 96
    obs = torch.zeros((rows + extra, W))
    obs[:, :obs_dim] = torch.rand((rows + extra, obs_dim), generator=g) * 2 - 1
    noise = torch.randn((rows + extra, 7), generator=g)
    obs, noise = obs.to(DEV), noise.to(DEV)
    obs_nan, noise_nan = obs.clone(), noise.clone()
    obs_nan[rows:, :obs_dim] = NAN
    noise_nan[rows:] = NAN
    sizes = {"mean": rows * 7, "value": rows, "action": rows * 7, "clipped": rows * 7, "log_prob": rows}
    runs = []
    for o, z in ((obs, noise), (obs_nan, noise_nan)):
        outs = {name: _guarded(cnt) for name, cnt in sizes.items()}
        k.forward(o[:rows], noise=z[:rows], **{name: (t[:sizes[name]].view(rows, 7) if sizes[name] == rows * 7 else t[:rows]) for name, t in outs.items()})
        torch.cuda.synchronize()
        for name, t in outs.items():
            assert _guard_intact(t, sizes[name]), name
            assert torch.isfinite(t[:sizes[name]]).all(), name
        runs.append({name: t[:sizes[name]].clone() for name, t in outs.items()})
    for name in sizes:
        assert torch.equal(runs[0][name], runs[1][name]), name
    k.close()


# ================================================================================================ 3. the clip coefficient
@pytest.mark.parametrize("kind", S.KINDS, ids=S.KIND_IDS)
def test_clip_coefficient_of_both_norm_routes_against_fp64(kind):
    """From m = v = 0 the kernel's exp_avg is exactly fl(0.1f * fl(g * c)), so it shows the clip coefficient c element by element.
    c_ref = min(M / (S + 1e-6), 1) in fp64, S from the device's own gradient read back; M = S / 2 (clipped) and 4 S (not clipped).
        |exp_avg - 0.1f * g * c_ref| <= 8 * 2^-24 * |0.1f * g * c_ref|
    (five fp32 roundings of at most 2^-24 each: the norm to float, + 1e-6f, the divide, g * c, 0.1f * gi; margin rounded up to eight).
    Every tensor of the spec holds >= 1e-4 of S^2 (asserted here and, on the fp64 torch gradient, by the CPU companion), so a norm that
    missed one tensor -- or counted the padded half of the 2x64 layout -- would move c by >= 5e-5, a hundred times the bound."""
    hidden, obs_dim, _ = kind
    c = S.CLIP_NORM
    pol, buf, sel = S.clip_norm_case(hidden, obs_dim)
    k = _handle(kind)
    flat = pol.flat.to(DEV)
    k.pack(flat)
    b, idx, n = _dev(buf), sel.to(DEV), c["n"]
    grad, stats = torch.full((k.num_params,), NAN, device=DEV), torch.zeros(4, device=DEV)
    over = dict(clip_range=c["clip_range"], ent_coef=c["ent_coef"], vf_coef=c["vf_coef"])
    k.set_step_count(0)
    _loss_grad(k, b, idx, n, grad, stats, **over)
    g = grad.cpu().double()
    assert torch.isfinite(g).all()
    shares = S.norm_shares(g, pol.spec)
    assert min(shares.values()) >= S.MIN_SHARE, shares
    Snorm = math.sqrt(float((g * g).sum()))
    tenth = float(np.float32(0.1))
    worst = {}
    for case, M in (("clipped", 0.5 * Snorm), ("not clipped", 4.0 * Snorm)):
        c_ref = min(M / (Snorm + 1e-6), 1.0)
        assert (c_ref < 0.51) if case == "clipped" else (c_ref == 1.0)
        ref = tenth * g * c_ref
        for route in (True, False):
            p, m, v = flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)
            k.adam_step(p, grad, m, v, lr=3e-4, eps=1e-5, max_grad_norm=M, step=0, fused_norm=route)
            torch.cuda.synchronize()
            rel = ((m.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
            worst[(case, "fused_norm" if route else "separate")] = rel
            k.pack(flat)
    print(f"{kind}: S {Snorm:.6f} worst relative error of exp_avg {worst} (bound {8 * 2.0 ** -24:.3e})")
    assert all(r <= 8 * 2.0 ** -24 for r in worst.values()), worst
    k.close()


# ================================================================================================ 4. step count and moments
_PARITY = {}      # what the last run measured, per case (profiles/mlp_handle_state_parity.json is one MI355X run of it)


@pytest.mark.parametrize("c0", [0, 1000])
@pytest.mark.parametrize("kind", [S.KINDS[0], S.KINDS[4]], ids=[S.KIND_IDS[0], S.KIND_IDS[4]])
def test_four_adam_steps_on_the_device_count_against_fp64(kind, c0):
    """set_step_count(c0), then four loss_grad -> adam_step(step = 0, fused_norm = True) pairs on different minibatches of n = 200, 33, 200, 1
    rows (the ragged launches advance the counter too).  After each step p, m and v, per tensor of the spec, against plain fp64 on the CPU --
    clip with S_t, the m and v recurrences, p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps), t = c0 + 1 .. c0 + 4 -- fed the device's own
    gradients g_t, so only the optimiser is under test:
        |device - fp64| <= 8 * max(e32, ulp(max|tensor|)),   e32 = |the same recurrences in fp32 torch on the CPU - fp64|
    For c0 = 0 a count that is off by one in either direction violates this bound on every weight tensor (CPU companion).  At c0 = 1000 a
    shift of one is below the bound, so there the result must only meet it and differ from the c0 = 0 result.
    MI355X, worst e_dev / bound over the four steps and the tensors (profiles/mlp_handle_state_parity.json has them per tensor):
        2x256 fused  c0 = 0     p 4.3e-08 / 3.3e-07   m 6.7e-10 / 3.7e-09   v 5.2e-14 / 2.8e-13
        2x256 fused  c0 = 1000  p 5.1e-08 / 4.1e-07   m 1.2e-10 / 7.6e-10   v 2.3e-14 / 1.2e-13
        2x64  layer  c0 = 0     p 7.9e-09 / 6.4e-08   m 6.3e-10 / 3.7e-09   v 1.7e-17 / 9.6e-17
        2x64  layer  c0 = 1000  p 5.1e-08 / 3.6e-07   m 3.5e-10 / 1.9e-09   v 4.1e-13 / 1.8e-12"""
    hidden, obs_dim, _ = kind
    a = S.ADAM
    pol = S.policy(hidden, obs_dim)
    buf = _dev(S.sample_buffers(pol.flat, pol.spec, obs_dim, seed=a["seed"]))
    over = dict(clip_range=a["clip_range"], ent_coef=a["ent_coef"], vf_coef=a["vf_coef"])
    kw = dict(lr=a["lr"], eps=a["eps"], max_grad_norm=a["max_grad_norm"])

    def run(start):
        k = _handle(kind)
        flat = pol.flat.to(DEV)
        k.pack(flat)
        k.set_step_count(start)
        p, m, v = flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)
        grads, states = [], []
        for i, n in enumerate(a["ns"]):
            idx = S.selection(S.TOTAL, n, 90 + i).to(DEV)
            grad, stats = torch.full((k.num_params,), NAN, device=DEV), torch.zeros(4, device=DEV)
            _loss_grad(k, buf, idx, n, grad, stats, **({"normalize": False} if n == 1 else {}), **over)
            k.adam_step(p, grad, m, v, step=0, fused_norm=True, **kw)
            torch.cuda.synchronize()
            grads.append(grad.cpu())
            states.append((p.cpu(), m.cpu(), v.cpu()))
        k.close()
        return grads, states

    grads, states = run(c0)
    assert all(torch.isfinite(g).all() for g in grads)
    ref64 = S.adam_restatement(pol.flat, grads, c0=c0, dtype=torch.float64, **kw)
    ref32 = S.adam_restatement(pol.flat, grads, c0=c0, dtype=torch.float32, **kw)
    bounds = S.adam_bounds(ref64, ref32, pol.spec)
    errs = S.adam_errors(ref64, states, pol.spec)
    failures, record = [], {}
    for name, _ in pol.spec:
        for what in "pmv":
            e_dev = max(e[name][what] for e in errs)
            step = max(range(len(errs)), key=lambda s: errs[s][name][what] / bounds[s][name][what][1])
            e, (e32, bound) = errs[step][name][what], bounds[step][name][what]
            record[f"{name}:{what}"] = {"e_dev": e, "e32": e32, "bound": bound, "step": step + 1, "e_dev_max": e_dev}
            print(f"  c0={c0} {name:36s} {what} step {step + 1}: device {e:.3e} fp32 torch {e32:.3e} bound {bound:.3e}")
            if any(not errs[s][name][what] <= bounds[s][name][what][1] for s in range(len(errs))):
                failures.append((name, what, e, bound))
    _PARITY[f"{S.KIND_IDS[S.KINDS.index(kind)]}:c0={c0}"] = record
    assert not failures, failures
    if c0 != 0:
        _, base = run(0)
        assert all((s[0] != b[0]).any() for s, b in zip(states, base))      # other bias corrections: another trajectory from step 1 on


# ================================================================================================ 5. batch-size edges
EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129]
EDGE_CASES = [(kd, n, 512) for kd in S.KINDS for n in EDGES]
EDGE_CASES += [(kd, 2080, 2176) for kd in S.KINDS if kd[2] == "fused"]        # 65 tiles: the last dW2 and dW1 chunks partly filled
EDGE_CASES += [(S.KINDS[2], n, 8192) for n in (6336, 6337)]                    # 99 / 100 row tiles of 64: launch_nt's tile-shape switch


@pytest.fixture(scope="module")
def edge_world():
    """per (kind, max_batch): one handle, reused by every n (as training reuses it), with its policy and sample buffers"""
    cache = {}

    def get(kind, max_batch):
        if (kind, max_batch) not in cache:
            hidden, obs_dim, _ = kind
            pol = S.policy(hidden, obs_dim)
            total = max(S.TOTAL, max_batch)
            buf = S.sample_buffers(pol.flat, pol.spec, obs_dim, total=total, seed=11)
            k = _handle(kind, max_batch=max_batch)
            cache[(kind, max_batch)] = (k, pol, buf, _dev(buf), total)
        k, pol, buf, dbuf, total = cache[(kind, max_batch)]
        k.pack(pol.flat.to(DEV))
        return k, pol, buf, dbuf, total

    yield get
    for k, *_ in cache.values():
        k.close()


def _check_grad(grad, stats, ref, spec, what, klb):
    g = grad.cpu().double()
    worst = 0.0
    for name, sl in S.slices_of(spec).items():
        scale = ref["grad"][sl].abs().max().item() + 1e-12
        err = (g[sl] - ref["grad"][sl]).abs().max().item()
        worst = max(worst, err / (2e-4 * scale + 1e-7))
        assert err <= 2e-4 * scale + 1e-7, f"{what} {name}: err {err} scale {scale}"
    st = stats.cpu().double()
    assert abs(st[0].item() - ref["policy_loss"]) <= 1e-4 * (abs(ref["policy_loss"]) + 1), what
    assert abs(st[1].item() - ref["value_loss"]) <= 1e-4 * (abs(ref["value_loss"]) + 1), what
    assert abs(st[2].item() - ref["entropy"]) <= 1e-5, what
    assert abs(klb["kl64"] - ref["approx_kl"]) <= 1e-12 * abs(ref["approx_kl"]), what
    return worst, _check_kl(st[3].item(), klb, what)


@pytest.mark.parametrize("kind,n,max_batch", EDGE_CASES, ids=[f"{S.KIND_IDS[S.KINDS.index(kd)]}-n{n}" for kd, n, _ in EDGE_CASES])
def test_batch_size_edges_against_fp64_autograd(edge_world, kind, n, max_batch):
    """loss_grad and forward at n rows against torch autograd in fp64 on the CPU, under the project's tolerances for this comparison
    (gradient per tensor 2e-4 * max|ref| + 1e-7, losses 1e-4 * (|x| + 1), forward rtol 1e-4 / atol 2e-5, 1e-4 for log_prob), and
    stats_out[3] against approx_kl in fp64 under _check_kl's bound, after one call and after two into the same buffer.  n >= 2:
    per-minibatch normalisation (SB3's unbiased std) and raw advantages; n = 1, where torch's std is NaN: raw and supplied statistics."""
    hidden, obs_dim, _ = kind
    k, pol, buf, dbuf, total = edge_world(kind, max_batch)
    sel = S.selection(total, n, 1000 + n)
    idx = sel.to(DEV)
    modes = [("raw", dict(normalize=False), None)]
    if n >= 2:
        modes.append(("minibatch", {}, None))
    else:
        given = (0.37, 1.9)
        modes.append(("given", dict(adv_stats=torch.tensor(given, device=DEV)), given))
    klb = R.approx_kl_bound(pol.flat, pol.spec, obs_dim, buf["obs"][sel], buf["act"][sel], buf["old_logp"][sel])
    for mode, extra, given in modes:
        ref = S.reference(pol.flat, pol.spec, obs_dim, buf, sel, adv_mode=mode, adv_stats=given, **KW)
        grad, stats = torch.full((k.num_params,), NAN, device=DEV), torch.zeros(4, device=DEV)
        _loss_grad(k, dbuf, idx, n, grad, stats, **extra)
        worst, kl = _check_grad(grad, stats, ref, pol.spec, (kind, n, mode), klb)
        print(f"{kind} n={n} {mode}: worst gradient error / tolerance {worst:.3f}, approx_kl {stats[3].item():.6e} error / bound {kl:.3f}")
    # stats_out accumulates: a second call into the same buffer leaves twice one call's approx_kl
    one = stats[3].item()
    _loss_grad(k, dbuf, idx, n, grad, stats, **extra)
    assert abs(stats[3].item() - 2 * one) <= klb["bound"], (kind, n, stats[3].item(), one)
    _check_kl(stats[3].item(), klb, (kind, n, "two calls"), calls=2)
    # forward over the same rows
    obs = dbuf["obs"][idx].contiguous()
    noise = dbuf["noise"][idx].contiguous()
    mean, value, action, logp = (torch.full(s, NAN, device=DEV) for s in ((n, 7), (n,), (n, 7), (n,)))
    k.forward(obs, noise=noise, mean=mean, value=value, action=action, log_prob=logp)
    Pv = S.views_of(pol.flat.double(), pol.spec)
    ref_action = ref["mean"] + torch.exp(Pv["log_std"]) * buf["noise"][sel].double()
    ref_logp = P.gaussian_log_prob(ref_action, ref["mean"], Pv["log_std"])
    assert torch.allclose(mean.cpu().double(), ref["mean"], rtol=1e-4, atol=2e-5), (mean.cpu().double() - ref["mean"]).abs().max()
    assert torch.allclose(value.cpu().double(), ref["value"], rtol=1e-4, atol=2e-5), (value.cpu().double() - ref["value"]).abs().max()
    assert torch.allclose(logp.cpu().double(), ref_logp, rtol=1e-4, atol=1e-4), (logp.cpu().double() - ref_logp).abs().max()


@pytest.mark.parametrize("kind", S.KINDS, ids=S.KIND_IDS)
def test_normalised_advantage_of_a_single_row_is_zero(edge_world, kind):
    """Per-minibatch normalisation at n = 1: the kernels define the statistics as mean = adv, 1 / (0 + 1e-8), so the normalised advantage is
    0 and the gradient is finite and equal, bit for bit, to that of a zero raw advantage."""
    k, pol, buf, dbuf, total = edge_world(kind, 512)
    idx = S.selection(total, 1, 77).to(DEV)
    g_norm, g_zero = torch.full((k.num_params,), NAN, device=DEV), torch.full((k.num_params,), NAN, device=DEV)
    s_norm, s_zero = torch.zeros(4, device=DEV), torch.zeros(4, device=DEV)
    _loss_grad(k, dbuf, idx, 1, g_norm, s_norm)
    zero = {**dbuf, "adv": torch.zeros_like(dbuf["adv"])}
    _loss_grad(k, zero, idx, 1, g_zero, s_zero, normalize=False)
    assert torch.isfinite(g_norm).all() and (g_norm != 0).any()
    assert torch.equal(g_norm, g_zero) and torch.equal(s_norm, s_zero)
