"""The rollout-tail kernels of kp1_ppo.hip at their edges, through the C ABI: kp1_gae_scan (one row, one column, both block sizes of the
launcher, every done byte), kp1_gae_scan_replicas at the large block size, kp1_bootstrap_truncated on all sixteen done bytes,
kp1_adv_minibatch_sums without idx / with a short, a one-row and an exact last minibatch, kp1_adv_minibatch_stats on two workgroups; and the two refusals of the unit that need a device (a curriculum window above the maximum, a device
index past the last device).  test_ppo_kernels_gpu.py holds the one-shape tests of the same kernels; tolerances here are theirs."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from rl_brain_trainer_amd import native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GAMMA, LAM = 0.995, 0.95
DONE_BYTES = (0, 1, 2, 3, 4, 5, 6, 8, 9, 12)     # TERMINATED = 1, TRUNCATED = 2, SUCCESS = 4, INVALID = 8: 4, 8 and 12 end no episode


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gae_restatement(r, v, done, lv, gamma, lam, dtype):
    """test_gae_scan_vs_sb3_formula's numpy restatement of SB3's RolloutBuffer.compute_returns_and_advantage, in `dtype`; gamma and lambda
    are the float32 values the kernel is handed"""
    T, N = r.shape
    g = dtype(np.float32(gamma))
    gl = g * dtype(np.float32(lam)) if dtype is np.float64 else np.float32(gamma * lam)
    r, v, lv = r.astype(dtype), v.astype(dtype), lv.astype(dtype)
    d = (done & 3) != 0
    ref, lg = np.zeros((T, N), dtype=dtype), np.zeros(N, dtype=dtype)
    for t in reversed(range(T)):
        nv = lv if t == T - 1 else v[t + 1]
        nonterm = dtype(1.0) - d[t].astype(dtype)
        delta = r[t] + g * nv * nonterm - v[t]
        lg = delta + gl * nonterm * lg
        ref[t] = lg
    return ref, ref + v


def _gae_inputs(T, N, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    rew, val, last = torch.randn((T, N), generator=g), torch.randn((T, N), generator=g), torch.randn(N, generator=g)
    done = torch.tensor(DONE_BYTES, dtype=torch.uint8)[torch.randint(0, len(DONE_BYTES), (T, N), generator=g)]
    done[:, 0] = 1                      # a column that is done at every step
    if N > 1:                           # and one done at the last step only
        done[:, 1] = 0
        done[T - 1, 1] = 2
    return rew, val, done.contiguous(), last


@pytest.mark.parametrize("T,N", [(1, 1), (1, 65), (3, 64), (5, 257), (2, 16384), (2, 16385)])
def test_gae_scan_shapes_and_done_bytes(T, N):
    """N <= 16384 launches 64-thread blocks, N = 16385 256-thread ones.  A done byte ends the episode iff it has TERMINATED or TRUNCATED set
    (`done & 3`), so a kernel that tested `done != 0` fails on 4, 8 and 12.  Against the numpy fp32 restatement at its test's tolerances, and
    no further from the fp64 restatement than 4 x the fp32 restatement's own distance + 1e-6."""
    rew, val, done, last = _gae_inputs(T, N, 7 * T + N)
    if T * N >= 192:
        assert all(int((done[:, 2:] == b).sum()) > 0 for b in DONE_BYTES)
    d = [t.to(DEV) for t in (rew, val, done, last)]
    adv, ret = torch.full((T, N), float("nan"), device=DEV), torch.full((T, N), float("nan"), device=DEV)
    L = native.load()
    native.check(L.kp1_gae_scan(0, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), GAMMA, LAM, _p(adv), _p(ret), T, N, None))
    torch.cuda.synchronize()
    a, q = adv.cpu().numpy(), ret.cpu().numpy()
    args = (rew.numpy(), val.numpy(), done.numpy(), last.numpy(), GAMMA, LAM)
    a32, q32 = _gae_restatement(*args, np.float32)
    a64, q64 = _gae_restatement(*args, np.float64)
    assert np.allclose(a, a32, rtol=1e-5, atol=1e-5) and np.allclose(q, q32, rtol=1e-5, atol=1e-5)
    for name, got, f32, f64 in (("advantages", a, a32, a64), ("returns", q, q32, q64)):
        own, dev = np.abs(f32.astype(np.float64) - f64).max(), np.abs(got.astype(np.float64) - f64).max()
        print(f"T={T} N={N} {name}: kernel - fp64 {dev:.3e}, numpy fp32 - fp64 {own:.3e}")
        assert dev <= 4 * own + 1e-6, (name, dev, own)
    # the all-done column never looks ahead: A_t = r_t - V_t exactly
    assert np.array_equal(a[:, 0], (rew[:, 0] - val[:, 0]).numpy())


def test_gae_scan_replicas_equals_single_scans_at_the_large_block_size():
    """N = 16385 = 5 x 3277 columns (256-thread blocks; replica borders inside blocks), five (gamma, lambda) pairs: each replica's columns
    are bit-equal to a kp1_gae_scan of those columns with its two scalars, as include/kp1_ppo.h promises."""
    T, K, n = 3, 5, 3277
    N = K * n
    rew, val, done, last = (t.to(DEV) for t in _gae_inputs(T, N, 99))
    pairs = [(0.995, 0.95), (0.99, 0.9), (0.9, 1.0), (1.0, 0.8), (0.97, 0.0)]
    gl = torch.tensor(pairs, dtype=torch.float32, device=DEV).contiguous()
    adv, ret = torch.full((T, N), float("nan"), device=DEV), torch.full((T, N), float("nan"), device=DEV)
    L = native.load()
    native.check(L.kp1_gae_scan_replicas(0, _p(rew), _p(val), _p(done), _p(last), _p(gl), n, _p(adv), _p(ret), T, N, None))
    for r, (gamma, lam) in enumerate(pairs):
        cols = slice(r * n, (r + 1) * n)
        one = [t[:, cols].contiguous() for t in (rew, val, done)] + [last[cols].contiguous()]
        a1, q1 = torch.full((T, n), float("nan"), device=DEV), torch.full((T, n), float("nan"), device=DEV)
        native.check(L.kp1_gae_scan(0, _p(one[0]), _p(one[1]), _p(one[2]), _p(one[3]), gamma, lam, _p(a1), _p(q1), T, n, None))
        assert torch.equal(adv[:, cols], a1) and torch.equal(ret[:, cols], q1), r
    assert torch.isfinite(adv).all() and not torch.equal(adv[:, :n], adv[:, n:2 * n])


@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_bootstrap_truncated_on_every_done_byte(count):
    """Done bytes cycle through all sixteen values of the low four bits (starting at 2, so count = 1 is a truncated step).  Rewards change
    exactly where `(d & 2) && !(d & 1)` and are bit-identical elsewhere.  A changed reward is fl(r + fl(gamma * tv)) or, contracted,
    fl(r + gamma * tv): each rounding is at most half a float32 spacing at its own magnitude, so it lies within one spacing -- taken at the
    largest of |r|, |gamma tv| and |result| -- of r + gamma * tv in fp64."""
    g = torch.Generator(device="cpu").manual_seed(count)
    rew = torch.randn(count, generator=g)
    tv = (torch.randint(0, 2, (count,), generator=g) * 2 - 1) * (0.5 + 1.5 * torch.rand(count, generator=g))     # |tv| >= 0.5: a bootstrapped reward always moves
    done = ((torch.arange(count) + 2) % 16).to(torch.uint8)
    out, tv_dev, done_dev = rew.to(DEV), tv.to(DEV), done.to(DEV)
    L = native.load()
    native.check(L.kp1_bootstrap_truncated(0, _p(out), _p(tv_dev), _p(done_dev), GAMMA, count, _stream()))
    torch.cuda.synchronize()
    out = out.cpu()
    hit = ((done & 2) != 0) & ((done & 1) == 0)
    assert count < 16 or int(hit.sum()) >= count // 4 - 1
    changed = out.view(torch.int32) != rew.view(torch.int32)
    assert torch.equal(changed, hit), (changed ^ hit).nonzero().flatten().tolist()
    step = np.float64(np.float32(GAMMA)) * tv.numpy().astype(np.float64)
    ref = rew.numpy().astype(np.float64) + step
    mag = np.maximum(np.maximum(np.abs(rew.numpy().astype(np.float64)), np.abs(step)), np.abs(ref))
    err = np.abs(out.numpy().astype(np.float64) - ref)[hit.numpy()]
    assert (err <= np.spacing(mag.astype(np.float32)).astype(np.float64)[hit.numpy()]).all(), err.max()


@pytest.mark.parametrize("gather", [True, False], ids=["idx", "identity"])
@pytest.mark.parametrize("total,mb", [(700, 1000), (300, 1), (6000, 3000), (10000, 3000)])
def test_adv_minibatch_sums_edges(total, mb, gather):
    """idx = NULL (identity); one short minibatch (minibatch > total); 300 minibatches of one row (sum of squares = sum^2, exactly: the square
    of a float32 is exact in fp64); an exact multiple; and the ragged shape of test_adv_minibatch_sums_vs_torch.  That test's bounds: exact
    counts, 1e-9 relative on both sums."""
    g = torch.Generator(device="cpu").manual_seed(total + mb)
    adv = torch.randn(total, generator=g) * 2 + 0.3
    perm = torch.randperm(total, generator=g)
    n_mb = (total + mb - 1) // mb
    out = torch.full((n_mb + 1, 3), -7.0, dtype=torch.float64, device=DEV)           # one guard row
    adv_dev, idx = adv.to(DEV), perm.to(DEV) if gather else None
    L = native.load()
    native.check(L.kp1_adv_minibatch_sums(0, _p(adv_dev), _p(idx) if gather else None, total, mb, _p(out), _stream()))
    torch.cuda.synchronize()
    out = out.cpu()
    assert (out[n_mb] == -7.0).all()
    order = perm if gather else torch.arange(total)
    for b in range(n_mb):
        sel = adv[order[b * mb:(b + 1) * mb]].double()
        assert out[b, 2].item() == sel.numel() == min(mb, total - b * mb)
        assert abs(out[b, 0].item() - sel.sum().item()) <= 1e-9 * sel.abs().sum().item()
        assert abs(out[b, 1].item() - (sel * sel).sum().item()) <= 1e-9 * (sel * sel).sum().item()
        if mb == 1:
            assert out[b, 0].item() == sel.item() and out[b, 1].item() == sel.item() ** 2


def test_adv_minibatch_stats_on_two_workgroups():
    """65 minibatches (the kernel's workgroups hold 64, so the second one runs), the last one ragged: (mean, 1 / (std + 1e-8)) against the
    fp64 expression include/kp1_ppo.h documents, evaluated on the sums the device produced, and against torch on the rows themselves,
    under test_adv_minibatch_sums_vs_torch's bounds (1e-6 absolute on the mean, 1e-5 relative on the inverse)."""
    total, mb = 65 * 40 - 13, 40
    g = torch.Generator(device="cpu").manual_seed(65)
    adv = torch.randn(total, generator=g) * 2 + 0.3
    perm = torch.randperm(total, generator=g)
    n_mb = (total + mb - 1) // mb
    assert n_mb == 65
    sums = torch.zeros((n_mb, 3), dtype=torch.float64, device=DEV)
    stats = torch.full((n_mb + 1, 2), -7.0, dtype=torch.float32, device=DEV)          # one guard row
    adv_dev, perm_dev = adv.to(DEV), perm.to(DEV)
    L = native.load()
    native.check(L.kp1_adv_minibatch_sums(0, _p(adv_dev), _p(perm_dev), total, mb, _p(sums), _stream()))
    native.check(L.kp1_adv_minibatch_stats(0, _p(sums), n_mb, _p(stats), _stream()))
    torch.cuda.synchronize()
    s, st = sums.cpu().numpy(), stats.cpu().numpy()
    assert (st[n_mb] == -7.0).all()
    mean = s[:, 0] / s[:, 2]
    var = np.maximum((s[:, 1] - s[:, 2] * mean * mean) / np.maximum(s[:, 2] - 1.0, 1.0), 0.0)
    inv = 1.0 / (np.sqrt(var) + 1e-8)
    assert (np.abs(st[:n_mb, 0] - mean) <= 1e-6).all() and (np.abs(st[:n_mb, 1] - inv) <= 1e-5 * inv).all()
    for b in (0, 63, 64):
        sel = adv[perm[b * mb:(b + 1) * mb]].double()
        assert abs(st[b, 0] - sel.mean().item()) <= 1e-6 and abs(st[b, 1] - 1.0 / (sel.std().item() + 1e-8)) <= 1e-5 * st[b, 1]
    assert s[64, 2] == 27


def test_curriculum_window_above_the_maximum_is_refused():
    """the one argument check of kp1_curriculum_create_population behind the device selection (the other refusals of the unit need no device:
    test_ppo_unit_refusals_cpu.py); the largest window is accepted, nothing is allocated for the refused one"""
    L = native.load()
    max_window = native.header_int("KP1_CURRICULUM_MAX_WINDOW")
    stages = (C.c_int32 * 2)(0, 1)
    out = C.c_void_p()
    assert L.kp1_curriculum_create_population(0, 2, 0.8, max_window + 1, 5, 3, C.cast(stages, C.c_void_p), C.byref(out)) == -1
    assert L.kp1_last_error().decode() == "window_episodes exceeds KP1_CURRICULUM_MAX_WINDOW" and out.value is None
    native.check(L.kp1_curriculum_create_population(0, 2, 0.8, max_window, 5, 3, C.cast(stages, C.c_void_p), C.byref(out)))
    assert out.value
    native.check(L.kp1_curriculum_destroy(0, out))


def test_device_index_equal_to_the_device_count_is_refused():
    """every kind of entry point of the unit (a launch, a creator, a read, the monitor's creator) with acceptable arguments and the first device
    index past the last device: KP1_ERR_INVALID before anything is launched, allocated or copied"""
    L = native.load()
    count = torch.cuda.device_count()
    buf = torch.full((64,), -7.0, dtype=torch.float32, device=DEV)
    host = (C.c_char * 65536)()
    stages = (C.c_int32 * 1)(0)
    out = C.c_void_p()
    calls = [lambda: L.kp1_gae_scan(count, _p(buf), _p(buf), _p(buf), _p(buf), GAMMA, LAM, _p(buf), _p(buf), 1, 8, _stream()),
             lambda: L.kp1_adv_minibatch_stats(count, _p(buf), 1, _p(buf), _stream()),
             lambda: L.kp1_curriculum_observe(count, _p(buf), _p(buf), 64, 1, _stream()),
             lambda: L.kp1_curriculum_read(count, _p(buf), C.cast(host, C.c_void_p), _stream()),
             lambda: L.kp1_curriculum_create_population(count, 1, 0.8, 10, 5, 3, C.cast(stages, C.c_void_p), C.byref(out)),
             lambda: L.kp1_monitor_create(count, 1, 8, 100, 4, C.byref(out)),
             lambda: L.kp1_explained_variance(count, _p(buf), _p(buf), 1, 8, 8, _p(buf), _stream())]
    for call in calls:
        assert call() == -1 and L.kp1_last_error().decode() == "device index out of range"
    torch.cuda.synchronize()
    assert out.value is None and (buf == -7.0).all() and bytes(host) == bytes(65536)
