"""The Adam launch reads its bias corrections from a record that the launch in front of it leaves next to the device step counts, and sums
the clip-norm partials with batched loads.  These are behaviour pins -- every case holds before and after that change:

  1. one loss_grad -> adam_step on the device count at counts 1, 2, 1000, 100000 and three clip regimes against torch.optim.Adam
  2. the clip coefficient the update implies against the fp64 norm of the gradient read back, at every n_partials the handle widths give
  3. three optimiser steps captured into a graph and replayed twice equal six eager steps, bit for bit (the record advances inside the graph)
  4. a K = 3 population handle with a hyper-parameter table equals three single handles, bit for bit
  5. the teacher-anchor step (actor extra count != 0) followed by two PPO steps: every tensor follows its own step count
  6. the caller's step count (host-step form), also with an actor extra count

Tolerances are the ones of the existing Adam tests.  Parameters against torch.optim.Adam as test_ppo_kernels_gpu.test_adam_step_vs_torch
compares them, at its learning rate of 6e-6: one fp32 spacing of the tensor's largest magnitude (its 6e-8 at |p| ~ 0.5), plus 4e-5 lr for the
update itself -- the update is at most lr * 0.1 / sqrt(0.001) = 3.2 lr, and the kernel's fp32 corrections 1 - 0.999f^t carry the rounding of
0.999f (1.3e-5 of bc2 at t = 1, half of it after the root) where torch forms them in double.  Moments against plain fp64 with
8 * max(e32, ulp(max|tensor|)), e32 = |torch.optim.Adam in fp32 - fp64| (test_mlp_handle_state_gpu.py section 4,
test_population_anchor_gpu.py section 2); the clip coefficient with 8 * 2^-24 relative (test_mlp_handle_state_gpu.py section 3).
The handles are small (minibatches of 32 and 70 rows): nothing
here depends on the size of the workload.  Sum-of-squares partials per handle: 2x64 40 and 43, 2x128 95 and 101, 2x256 253 and 265 (obs 56
and 80) -- below 64, not multiples of 64, and more than 256, which takes a second batch of loads."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import mlp_handle_state as S

pytestmark = pytest.mark.gpu
DEV = S.DEV
NAN = float("nan")
KINDS = [(64, 56), (64, 80), (128, 56), (128, 80), (256, 56), (256, 80)]
IDS = [f"{h}-{d}" for h, d in KINDS]
LR, EPS = 6e-6, 1e-5


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


class _World:
    """one handle kind: policy, sample buffers on the device and a max_batch = 128 handle"""

    def __init__(self, kind):
        self.hidden, self.obs_dim = kind
        self.pol = S.policy(self.hidden, self.obs_dim)
        self.spec = self.pol.spec
        self.flat = self.pol.flat.to(DEV)
        self.buf = S.dev(S.sample_buffers(self.pol.flat, self.spec, self.obs_dim, seed=1))
        self.k = S.handle((self.hidden, self.obs_dim, "fused" if self.hidden == 256 else "layer"), max_batch=128)

    def grad_at(self, count: int, n: int, seed: int, extra: int = 0) -> torch.Tensor:
        """pack the start parameters, set the counts, one loss_grad (which advances the count to count + 1)"""
        self.k.pack(self.flat)
        self.k.set_step_count(count)
        self.k.set_actor_extra_steps(extra)
        grad, stats = torch.full((self.k.num_params,), NAN, device=DEV), torch.zeros(4, device=DEV)
        S.loss_grad(self.k, self.buf, S.selection(S.TOTAL, n, seed).to(DEV), n, grad, stats)
        return grad


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(kind) -> _World:
        if kind not in made:
            made[kind] = _World(kind)
        return made[kind]

    yield get
    for w in made.values():
        w.k.close()


# ------------------------------------------------------------------------------------------------ the references
def _adam_refs(spec, state, grad, t_of, *, lr, eps, M, names=None):
    """One clip_grad_norm_ + Adam step over the tensors `names` (all of the spec by default), tensor `name` at step count t_of[name], from
    state = (p, m, v) flat fp32 CPU tensors and the flat gradient.  Returns the step in plain fp64 and through torch.optim.Adam in fp32, each
    as (p, m, v) flat CPU tensors (tensors outside `names` unchanged).  M = 0: no clipping."""
    sl = S.slices_of(spec)
    names = list(sl) if names is None else list(names)
    g64 = grad.detach().cpu().double()
    norm = math.sqrt(sum(float((g64[sl[n]] * g64[sl[n]]).sum()) for n in names))
    c = min(M / (norm + 1e-6), 1.0) if M > 0 else 1.0
    p64, m64, v64 = (t.detach().cpu().double().clone() for t in state)
    for n in names:
        s, t = sl[n], t_of[n]
        g = g64[s] * c
        m64[s] = 0.9 * m64[s] + 0.1 * g
        v64[s] = 0.999 * v64[s] + 0.001 * g * g
        p64[s] = p64[s] - (lr / (1.0 - 0.9 ** t)) * m64[s] / (v64[s].sqrt() / math.sqrt(1.0 - 0.999 ** t) + eps)
    p32, m32, v32 = (t.detach().cpu().clone() for t in state)
    params = [torch.nn.Parameter(p32[sl[n]].clone()) for n in names]
    for prm, n in zip(params, names):
        prm.grad = grad.detach().cpu()[sl[n]].clone()
    if M > 0:
        torch.nn.utils.clip_grad_norm_(params, M)
    opt = torch.optim.Adam(params, lr=lr, eps=eps)
    for prm, n in zip(params, names):
        opt.state[prm] = {"step": torch.tensor(float(t_of[n] - 1)), "exp_avg": m32[sl[n]].clone(), "exp_avg_sq": v32[sl[n]].clone()}
    opt.step()
    for prm, n in zip(params, names):
        p32[sl[n]], m32[sl[n]], v32[sl[n]] = prm.data, opt.state[prm]["exp_avg"], opt.state[prm]["exp_avg_sq"]
    return (p64, m64, v64), (p32, m32, v32)


def _failures(spec, what, dev, ref64, ref32, lr=LR) -> list:
    """p against torch.optim.Adam's, m and v against fp64 (the module docstring has the bounds)"""
    out = []
    for name, sl in S.slices_of(spec).items():
        e_p = (dev[0][sl].detach().cpu().double() - ref32[0][sl].double()).abs().max().item()
        b_p = float(np.spacing(np.float32(ref32[0][sl].abs().max().item()))) + 4e-5 * lr
        if not e_p <= b_p:
            out.append((what, name, "p", e_p, b_p))
        for tag, d, r, f in zip("mv", dev[1:], ref64[1:], ref32[1:]):
            e_dev = (d[sl].detach().cpu().double() - r[sl]).abs().max().item()
            e32 = (f[sl].double() - r[sl]).abs().max().item()
            bound = 8.0 * max(e32, float(np.spacing(np.float32(r[sl].abs().max().item()))))
            if not e_dev <= bound:
                out.append((what, name, tag, e_dev, e32, bound))
    return out


# ================================================================================================ 1. against torch.optim.Adam
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_device_step_against_torch_adam(worlds, kind):
    """loss_grad (advances the count to t) -> adam_step(step = 0, fused_norm) from m = v = 0 at t = 1, 2, 1000, 100000, with max_grad_norm four
    times the gradient's norm (coefficient exactly 1), a fiftieth of it, and 0 (no clipping); minibatches of 32 and 70 rows in turn."""
    w = worlds(kind)
    bad, worst = [], 0.0
    for i, t in enumerate((1, 2, 1000, 100000)):
        n = (32, 70)[i % 2]
        grad = w.grad_at(t - 1, n, seed=40 + i)
        norm = float(grad.double().norm())
        assert math.isfinite(norm) and norm > 0
        for regime, M in (("below", 4.0 * norm), ("above", norm / 50.0), ("off", 0.0)):
            p, m, v = w.flat.clone(), torch.zeros_like(w.flat), torch.zeros_like(w.flat)
            w.k.adam_step(p, grad, m, v, lr=LR, eps=EPS, max_grad_norm=M, step=0, fused_norm=True)
            torch.cuda.synchronize()
            zero = torch.zeros(w.k.num_params)
            ref64, ref32 = _adam_refs(w.spec, (w.flat, zero, zero), grad, dict.fromkeys(S.slices_of(w.spec), t), lr=LR, eps=EPS, M=M)
            bad += _failures(w.spec, (t, n, regime), (p, m, v), ref64, ref32)
            worst = max(worst, (p.cpu() - ref32[0]).abs().max().item())
            assert not torch.equal(p, w.flat)
            if regime == "below":       # coefficient exactly 1: the same bits as without clipping
                unclipped = [x.clone() for x in (p, m, v)]
            if regime == "off":
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(unclipped, (p, m, v)))
    print(f"{kind}: worst |p - torch.optim.Adam| {worst:.3e}")
    assert not bad, bad


def test_a_count_rewritten_by_the_host_gives_the_bits_of_the_record(worlds):
    """adam_step right behind loss_grad (the record's counts are the device's) and the same step after set_step_count has rewritten the count
    to the same value, and to another one and back: equal bits.  A different count gives different parameters."""
    w = worlds((128, 80))
    grad = w.grad_at(6, 70, seed=3, extra=2)

    def step(count=None):
        if count is not None:
            w.k.set_step_count(count)
        p, m, v = w.flat.clone(), torch.zeros_like(w.flat), torch.zeros_like(w.flat)
        w.k.adam_step(p, grad, m, v, lr=LR, eps=EPS, max_grad_norm=0.5, step=0, fused_norm=True)
        torch.cuda.synchronize()
        return p

    first = step()
    assert torch.equal(_bits(step(7)), _bits(first))
    other = step(8)
    assert not torch.equal(other, first)
    assert torch.equal(_bits(step(7)), _bits(first))
    w.k.set_actor_extra_steps(3)
    assert not torch.equal(step(), first)
    w.k.set_actor_extra_steps(2)
    assert torch.equal(_bits(step()), _bits(first))


# ================================================================================================ 2. the clip norm
@pytest.mark.parametrize("n", [32, 70])
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_clip_coefficient_at_every_partial_count(worlds, kind, n):
    """From m = 0 the kernel's exp_avg is exactly fl(0.1f * fl(g * c)), so it shows the clip coefficient c element by element:
        |exp_avg - 0.1f * g * c_ref| <= 8 * 2^-24 * |0.1f * g * c_ref|,   c_ref = M / (S + 1e-6), M = S / 2, S the fp64 norm of the gradient
    read back (five fp32 roundings of at most 2^-24; test_mlp_handle_state_gpu.py section 3).  Both norm routes: the finalize launch's
    partials (their number depends on the handle's widths) and the separate reduction's.  A partial left out, or the last one counted twice,
    moves c by half that block's share of S^2."""
    w = worlds(kind)
    grad = w.grad_at(0, n, seed=60 + n)
    g = grad.cpu().double()
    Snorm = math.sqrt(float((g * g).sum()))
    M = 0.5 * Snorm
    ref = float(np.float32(0.1)) * g * (M / (Snorm + 1e-6))
    for route in (True, False):
        p, m, v = w.flat.clone(), torch.zeros_like(w.flat), torch.zeros_like(w.flat)
        w.k.adam_step(p, grad, m, v, lr=LR, eps=EPS, max_grad_norm=M, step=0, fused_norm=route)
        torch.cuda.synchronize()
        rel = ((m.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
        print(f"{kind} n={n} fused_norm={route}: S {Snorm:.6f} worst relative error of exp_avg {rel:.3e} (bound {8 * 2.0 ** -24:.3e})")
        assert rel <= 8 * 2.0 ** -24, (route, rel)


# ================================================================================================ 3. graph replay
@pytest.mark.parametrize("kind", [(128, 80), (256, 56)], ids=["128-80", "256-56"])
def test_three_captured_steps_replayed_twice_equal_six_eager_steps(worlds, kind):
    w = worlds(kind)
    k = w.k
    ns = (70, 32, 70)
    idx = [S.selection(S.TOTAL, n, 80 + i).to(DEV) for i, n in enumerate(ns)]
    p, m, v = w.flat.clone(), torch.zeros_like(w.flat), torch.zeros_like(w.flat)
    grad, stats = torch.empty(k.num_params, device=DEV), torch.zeros(4, device=DEV)
    rows = w.buf["obs"][:96].contiguous()

    def three():
        for n, ix in zip(ns, idx):
            S.loss_grad(k, w.buf, ix, n, grad, stats)
            k.adam_step(p, grad, m, v, lr=LR, eps=EPS, max_grad_norm=0.5, step=0, fused_norm=True)

    def start():
        p.copy_(w.flat), m.zero_(), v.zero_(), stats.zero_()
        k.pack(p)
        k.set_step_count(0)
        k.set_actor_extra_steps(0)
        torch.cuda.synchronize()

    def result():
        """p, m, v, what the packed weights compute, and a probe of the device count: one more Adam step on scratch tensors"""
        torch.cuda.synchronize()
        mean, value = torch.empty((96, 7), device=DEV), torch.empty(96, device=DEV)
        k.forward(rows, mean=mean, value=value)
        pp, pm, pv = w.flat.clone(), torch.zeros_like(w.flat), torch.zeros_like(w.flat)
        k.adam_step(pp, grad, pm, pv, lr=LR, eps=EPS, max_grad_norm=0.5, step=0, fused_norm=False)
        torch.cuda.synchronize()
        return [t.clone() for t in (p, m, v, stats, mean, value, pp)]

    start()
    three()
    three()
    eager = result()
    start()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        three()
    start()
    graph.replay()
    graph.replay()
    replayed = result()
    for name, a, b in zip(("p", "m", "v", "stats", "mean", "value", "count probe"), eager, replayed):
        assert torch.equal(_bits(a), _bits(b)), (kind, name)
    assert torch.isfinite(eager[0]).all() and not torch.equal(eager[0], w.flat)
    # the probe does see the count: the same probe at an explicitly set count of 6 is equal, at 5 it is not
    for count, same in ((6, True), (5, False)):
        k.set_step_count(count)
        pp, pm, pv = w.flat.clone(), torch.zeros_like(w.flat), torch.zeros_like(w.flat)
        k.adam_step(pp, grad, pm, pv, lr=LR, eps=EPS, max_grad_norm=0.5, step=0, fused_norm=False)
        torch.cuda.synchronize()
        assert torch.equal(pp, eager[6]) == same, count


# ================================================================================================ 4. population
@pytest.mark.parametrize("hidden,obs_dim", [(64, 80), (128, 56)])
def test_population_with_a_table_equals_single_handles(hidden, obs_dim):
    """K = 3, per-replica learning rate, eps and max_grad_norm (one clips hard, one never), counts 999 + 2 actor extra steps, two steps of 70
    and 32 rows: replica k equals a K = 1 handle given entry k's scalars, bit for bit (one record serves all replicas)."""
    from rl_brain_trainer_amd.mlp import MlpKernels

    K = 3
    table = [dict(learning_rate=3e-4, adam_eps=1e-5, max_grad_norm=1e-3, clip_range=0.2, ent_coef=1e-3, vf_coef=0.5),
             dict(learning_rate=1e-3, adam_eps=1e-6, max_grad_norm=1e6, clip_range=0.1, ent_coef=0.0, vf_coef=0.25),
             dict(learning_rate=5e-5, adam_eps=1e-4, max_grad_norm=0.5, clip_range=0.3, ent_coef=0.05, vf_coef=1.0)]
    pols = [S.policy(hidden, obs_dim, seed=3 + 10 * r) for r in range(K)]
    spec = pols[0].spec
    flat = torch.stack([p.flat for p in pols]).to(DEV).contiguous()
    buf = S.dev(S.sample_buffers(pols[0].flat, spec, obs_dim, seed=2))
    ns = (70, 32)
    idx = [torch.stack([S.selection(S.TOTAL, n, 500 + 10 * i + r) for r in range(K)]).to(DEV).contiguous() for i, n in enumerate(ns)]

    def run(k, f, ix, scalars):
        k.pack(f)
        k.set_step_count(999)
        k.set_actor_extra_steps(2)
        p, m, v = f.clone(), torch.zeros_like(f), torch.zeros_like(f)
        grad, stats = torch.empty_like(f), torch.zeros((f.shape[0] if f.dim() == 2 else 1, 4), device=DEV)
        for n, i in zip(ns, ix):
            k.loss_grad(buf["obs"], i, n, buf["act"], buf["old_logp"], buf["adv"], buf["ret"], clip_range=scalars["clip_range"],
                        ent_coef=scalars["ent_coef"], vf_coef=scalars["vf_coef"], inv_count=1.0 / n, grad_out=grad, stats_out=stats)
            k.adam_step(p, grad, m, v, lr=scalars["learning_rate"], eps=scalars["adam_eps"], max_grad_norm=scalars["max_grad_norm"], step=0,
                        fused_norm=True)
        torch.cuda.synchronize()
        return p, m, v, grad, stats

    pop = MlpKernels(hidden, DEV, max_batch=128, obs_dim=obs_dim, replicas=K)
    pop.set_replica_hparams(table)
    shared = dict(learning_rate=0.1, adam_eps=0.5, max_grad_norm=100.0, clip_range=0.9, ent_coef=0.7, vf_coef=3.0)    # ignored with a table
    out = run(pop, flat, idx, shared)
    pop.close()
    assert float(out[3][0].double().norm()) > 10 * table[0]["max_grad_norm"]
    for r, h in enumerate(table):
        one = MlpKernels(hidden, DEV, max_batch=128, obs_dim=obs_dim)
        got = run(one, flat[r].contiguous(), [i[r].contiguous() for i in idx], h)
        one.close()
        for name, a, b in zip(("p", "m", "v", "grad", "stats"), got, out):
            assert torch.equal(_bits(a.reshape(-1)), _bits(b[r].reshape(-1))), (name, r)
        assert not torch.equal(got[0], flat[r])


# ================================================================================================ 5. teacher-anchor
from rl_brain_trainer_amd.teacher_anchor import ACTOR_TENSORS as ACTOR      # noqa: E402  (the six tensors torch's anchor step updates)


@pytest.mark.parametrize("kind", [(64, 56), (128, 80)], ids=["64-56", "128-80"])
def test_anchor_step_then_two_ppo_steps_follow_their_own_counts(worlds, kind):
    """Counts (4, 2): the anchor step moves the six actor tensors at t = 4 + 2 + 1 = 7 and raises the extra count to 3; the PPO step behind it
    runs at t = 5 and 5 + 3 = 8 for the actor tensors, the next one, with no anchor step in between, at 6 and 9.  After each of the three steps
    every tensor against one torch.optim.Adam step with per-tensor step counts (and its fp64 restatement) fed the device's own gradient."""
    w = worlds(kind)
    k, spec = w.k, w.spec
    assert set(ACTOR) <= set(S.slices_of(spec))
    g = torch.Generator(device="cpu").manual_seed(23)
    teacher = torch.randn((S.TOTAL, 7), generator=g).to(DEV).contiguous()
    k.pack(w.flat)
    k.set_step_count(4)
    k.set_actor_extra_steps(2)
    p = w.flat.clone()
    m, v = (1e-3 * torch.randn(k.num_params, generator=g)).to(DEV), (1e-6 * torch.rand(k.num_params, generator=g)).to(DEV)
    state = tuple(t.cpu().clone() for t in (p, m, v))
    grad, stats, loss = torch.empty(k.num_params, device=DEV), torch.zeros(4, device=DEV), torch.empty(1, device=DEV)
    bad = []

    def compare(what, t_of, M, names=None):
        nonlocal state
        torch.cuda.synchronize()
        ref64, ref32 = _adam_refs(spec, state, grad, t_of, lr=LR, eps=EPS, M=M, names=names)
        bad.extend(_failures(spec, what, (p, m, v), ref64, ref32))
        state = tuple(t.cpu().clone() for t in (p, m, v))      # the next step starts from the device's state

    k.anchor_loss_grad(w.buf["obs"], S.selection(S.TOTAL, 70, 7).to(DEV), 70, teacher, loss_weight=0.5, grad_out=grad, loss_out=loss)
    k.anchor_adam_step(p, grad, m, v, lr=LR, eps=EPS, max_grad_norm=0.5, step=0)
    compare("anchor", dict.fromkeys(ACTOR, 7), 0.5, names=ACTOR)
    rest = [n for n in S.slices_of(spec) if n not in ACTOR]
    for n in rest:      # nothing outside the actor tensors moved
        sl = S.slices_of(spec)[n]
        assert torch.equal(p[sl], w.flat[sl])
    for i, (common, actor) in enumerate(((5, 8), (6, 9))):
        n = (32, 70)[i]
        S.loss_grad(k, w.buf, S.selection(S.TOTAL, n, 30 + i).to(DEV), n, grad, stats)
        k.adam_step(p, grad, m, v, lr=LR, eps=EPS, max_grad_norm=0.5, step=0, fused_norm=True)
        compare(f"ppo step {i + 1}", {name: actor if name in ACTOR else common for name in S.slices_of(spec)}, 0.5)
    assert not bad, bad
    k.pack(w.flat)


# ================================================================================================ 6. the caller's step count
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("kind", [(64, 80), (256, 56)], ids=["64-80", "256-56"])
def test_host_step_form_against_torch_adam(worlds, kind, extra):
    """adam_step(step = t) for t = 1 and 1000 while the device count holds something else; with an actor extra count the kernel forms the
    actor tensors' corrections itself"""
    w = worlds(kind)
    bad = []
    for t in (1, 1000):
        grad = w.grad_at(76, 70, seed=90 + t, extra=extra)      # the device count is 77 now
        p, m, v = w.flat.clone(), torch.zeros_like(w.flat), torch.zeros_like(w.flat)
        w.k.adam_step(p, grad, m, v, lr=LR, eps=EPS, max_grad_norm=0.5, step=t, fused_norm=True)
        torch.cuda.synchronize()
        zero = torch.zeros(w.k.num_params)
        t_of = {name: t + extra if name in ACTOR else t for name in S.slices_of(w.spec)}
        ref64, ref32 = _adam_refs(w.spec, (w.flat, zero, zero), grad, t_of, lr=LR, eps=EPS, M=0.5)
        bad += _failures(w.spec, (t, extra), (p, m, v), ref64, ref32)
    w.k.set_actor_extra_steps(0)
    w.k.pack(w.flat)
    assert not bad, bad
