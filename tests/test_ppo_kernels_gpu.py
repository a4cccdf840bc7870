"""PPO-side HIP kernels vs plain PyTorch fp32 references of the same ops (SB3 semantics are 'parity unpinned':
SB3 2.8.0 is not in the reference tree or this image; see include/kp1_ppo.h).

Tolerances (fp32): the MFMA path sums K in a different order than torch/rocBLAS, so forward values agree to
~1e-5 relative and gradients to ~2e-4 of their scale; both are written next to each assert."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import row_attribution as R
from conftest import load_golden_config
from rl_brain_trainer_amd import ppo as P
from rl_brain_trainer_amd.curriculum import PointCurriculum
from rl_brain_trainer_amd.mlp import MlpKernels
from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _policy(hidden=256, seed=3, scale_heads=True, obs_dim=56):
    pol = P.ActorCritic(hidden, DEV, seed=seed, obs_dim=obs_dim)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    # non-trivial biases / log_std so every gradient path is exercised
    for name, _ in pol.spec:
        if name.endswith("bias"):
            pol.views[name].copy_(0.1 * torch.randn(pol.views[name].shape, generator=g))
    pol.views["log_std"].copy_(torch.tensor([-0.3, 0.1, -0.5, 0.0, 0.2, -0.1, -0.7]))
    if scale_heads:
        pol.views["action_net.weight"].mul_(30.0)
    return pol


@pytest.mark.parametrize("obs_dim", [56, 80])
def test_fused_tile_kernel_matches_layerwise_kernels_and_is_reproducible(obs_dim):
    """Same minibatch through mlp_train_tile_kernel and through gemm_nt x3 + head_train: the GEMM k-order is identical, only
    the per-tile partial sums differ in grouping (32- vs 64-row tiles), so gradients agree to a few fp32 ulps of their scale;
    two runs of the fused path are bitwise equal (no float atomics)."""
    D, W = obs_dim, (64 if obs_dim <= 64 else 128)
    pol = _policy(scale_heads=False, obs_dim=D)
    k = MlpKernels(256, DEV, max_batch=8192, obs_dim=D)
    k.pack(pol.flat)
    g = torch.Generator(device=DEV).manual_seed(5)
    total, n = 30000, 8000          # ragged last tile (8000 = 250 * 32) and a gather
    obs = torch.zeros((total, W), device=DEV)
    obs[:, :D] = torch.rand((total, D), device=DEV, generator=g) * 2 - 1
    act = torch.randn((total, 7), device=DEV, generator=g) * 0.5
    old_logp = -7.0 + 0.3 * torch.randn(total, device=DEV, generator=g)
    adv = torch.randn(total, device=DEV, generator=g)
    ret = torch.randn(total, device=DEV, generator=g)
    idx = torch.randperm(total, device=DEV, generator=g)[:n]
    out = {}
    for name, fused in (("fused", True), ("fused2", True), ("layer", False)):
        k.set_fused(fused)
        grad = torch.full((k.num_params,), float("nan"), device=DEV)
        stats = torch.zeros(4, device=DEV)
        k.loss_grad(obs, idx, n, act, old_logp, adv, ret, clip_range=0.2, ent_coef=1e-3, vf_coef=0.5, inv_count=1.0 / n, grad_out=grad, stats_out=stats)
        out[name] = (grad.clone(), stats.clone())
    assert torch.equal(out["fused"][0], out["fused2"][0]) and torch.equal(out["fused"][1], out["fused2"][1])
    gf, gl = out["fused"][0], out["layer"][0]
    assert torch.isfinite(gf).all()
    off = 0
    for name, shape in pol.spec:
        cnt = math.prod(shape)
        a, b = gf[off:off + cnt], gl[off:off + cnt]
        scale = b.abs().max().item() + 1e-12
        assert (a - b).abs().max().item() <= 2e-5 * scale + 1e-9, name
        off += cnt
    assert torch.allclose(out["fused"][1], out["layer"][1], rtol=1e-5, atol=1e-6)
    k.close()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("n,stride", [(4096, 56), (4096, 64), (100, 56), (8192, 64), (12000, 64), (1, 64),
                                      (4096, 80), (8192, 128), (100, 80), (1, 128)])   # 80 / 128: route observation (80 floats, pitch 128)
def test_mlp_forward_vs_torch(n, stride, fused):
    D = 56 if stride <= 64 else 80
    pol = _policy(obs_dim=D)
    k = MlpKernels(256, DEV, max_batch=16384, obs_dim=D)
    k.set_fused(fused)
    k.pack(pol.flat)
    g = torch.Generator(device=DEV).manual_seed(0)
    obs = torch.rand((n, stride), device=DEV, generator=g) * 2 - 1
    obs[:, D:] = 0
    noise = torch.randn((n, 7), device=DEV, generator=g)
    mean = torch.empty((n, 7), device=DEV)
    value = torch.empty(n, device=DEV)
    action = torch.empty((n, 7), device=DEV)
    clipped = torch.empty((n, 7), device=DEV)
    logp = torch.empty(n, device=DEV)
    k.forward(obs, noise=noise, mean=mean, value=value, action=action, clipped=clipped, log_prob=logp)
    ref_mean, ref_value = P.mlp_forward(pol.views, obs[:, :D].contiguous())
    assert torch.allclose(mean, ref_mean, rtol=1e-4, atol=2e-5), (mean - ref_mean).abs().max()
    assert torch.allclose(value, ref_value, rtol=1e-4, atol=2e-5), (value - ref_value).abs().max()
    ref_action = ref_mean + torch.exp(pol.views["log_std"]) * noise
    assert torch.allclose(action, ref_action, rtol=1e-4, atol=5e-5)
    assert torch.allclose(clipped, ref_action.clamp(-1, 1), rtol=1e-4, atol=5e-5)
    ref_logp = P.gaussian_log_prob(ref_action, ref_mean, pol.views["log_std"])
    assert torch.allclose(logp, ref_logp, rtol=1e-4, atol=1e-4)
    # single-output calls (the fused path launches only the net that is asked for)
    value2 = torch.empty(n, device=DEV)
    k.forward(obs, value=value2)
    assert torch.equal(value2, value)
    mean2 = torch.empty((n, 7), device=DEV)
    k.forward(obs, mean=mean2)
    assert torch.equal(mean2, mean)
    k.close()


# "bf16x3": the round-3 EXPERIMENT (KP1_MLP_OPT_BF16X3_WGRAD: weight-gradient GEMMs on operands split into three bf16 pieces) under the very same
# tolerances as the exact fp32 kernels -- the acceptance condition the round-2 review set for it
@pytest.mark.parametrize("fused", [True, False, "bf16x3"])
@pytest.mark.parametrize("obs_dim", [56, 80])
@pytest.mark.parametrize("n,total,gather", [(8192, 20000, True), (4096, 4096, False), (1000, 5000, True), (16384, 40000, True), (33, 64, True)])
def test_mlp_loss_grad_vs_torch_autograd(n, total, gather, fused, obs_dim):
    D, W = obs_dim, (64 if obs_dim <= 64 else 128)
    pol = _policy(scale_heads=False, obs_dim=D)
    k = MlpKernels(256, DEV, max_batch=16384, obs_dim=D)
    k.set_fused(bool(fused))
    if fused == "bf16x3":
        k.set_bf16x3_wgrad(True)
    k.pack(pol.flat)
    g = torch.Generator(device=DEV).manual_seed(1)
    obs = torch.zeros((total, W), device=DEV)
    obs[:, :D] = torch.rand((total, D), device=DEV, generator=g) * 2 - 1
    with torch.no_grad():
        m0, v0 = P.mlp_forward(pol.views, obs[:, :D].contiguous())
    act = m0 + torch.exp(pol.views["log_std"]) * torch.randn((total, 7), device=DEV, generator=g)
    # old log-probs from a slightly different policy so ratios spread around 1 and both clip branches occur
    old_logp = P.gaussian_log_prob(act, m0 + 0.05 * torch.randn((total, 7), device=DEV, generator=g), pol.views["log_std"])
    adv = torch.randn(total, device=DEV, generator=g) * 3 + 0.5
    ret = v0 + torch.randn(total, device=DEV, generator=g)
    idx = torch.randperm(total, device=DEV, generator=g)[:n] if gather else None
    clip, ent, vf = 0.1, 3e-4, 0.5
    grad = torch.empty(k.num_params, device=DEV)
    stats = torch.zeros(4, device=DEV)
    k.loss_grad(obs, idx, n, act, old_logp, adv, ret, clip_range=clip, ent_coef=ent, vf_coef=vf, inv_count=1.0 / n, grad_out=grad, stats_out=stats)

    # reference: SB3's loss with torch autograd
    sel = idx if gather else torch.arange(n, device=DEV)
    flat = pol.flat.detach().clone().requires_grad_(True)
    Pv, off = {}, 0
    for name, shape in pol.spec:
        cnt = math.prod(shape)
        Pv[name] = flat[off:off + cnt].view(shape)
        off += cnt
    mean, value = P.mlp_forward(Pv, obs[sel, :D])
    logp = P.gaussian_log_prob(act[sel], mean, Pv["log_std"])
    a = adv[sel]
    a = (a - a.mean()) / (a.std() + 1e-8)
    ratio = torch.exp(logp - old_logp[sel])
    pl = -torch.min(a * ratio, a * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    vl = torch.nn.functional.mse_loss(ret[sel], value)
    entropy = (0.5 + 0.5 * math.log(2 * math.pi) + Pv["log_std"]).sum()
    loss = pl + ent * (-entropy) + vf * vl
    (ref,) = torch.autograd.grad(loss, flat)
    frac_clipped = ((ratio - 1).abs() > clip).float().mean().item()
    if n >= 1000:
        assert 0.02 < frac_clipped < 0.98      # both branches of the surrogate are exercised
    off = 0
    for name, shape in pol.spec:
        cnt = math.prod(shape)
        gk, gr = grad[off:off + cnt], ref[off:off + cnt]
        scale = gr.abs().max().item() + 1e-12
        err = (gk - gr).abs().max().item()
        assert err <= 2e-4 * scale + 1e-7, f"{name}: err {err} scale {scale}"
        off += cnt
    assert abs(stats[0].item() - pl.item()) <= 1e-4 * (abs(pl.item()) + 1)
    assert abs(stats[1].item() - vl.item()) <= 1e-4 * (abs(vl.item()) + 1)
    assert abs(stats[2].item() - entropy.item()) <= 1e-5
    # stats_out[3] = approx_kl = mean((ratio - 1) - log ratio), against fp64 on the CPU.  No project tolerance exists for it: the bound is
    # 8 * max(e32, floor), e32 the error of the same expression in float32 torch on the CPU, floor = 2^-23 * max(1, max|logp|) * mean|log ratio|
    # (the log ratio inherits one fp32 spacing of the log-prob and d kl / d log ratio ~ log ratio; tests/row_attribution.py)
    klb = R.approx_kl_bound(pol.flat, pol.spec, D, obs[sel], act[sel], old_logp[sel])
    kl_err = abs(stats[3].item() - klb["kl64"])
    print(f"approx_kl {stats[3].item():.6e} fp64 {klb['kl64']:.6e}: error {kl_err:.3e} / bound {klb['bound']:.3e} = {kl_err / klb['bound']:.3f}")
    assert klb["kl64"] > 100 * klb["bound"], klb       # so that a missing inv_count, another slot or a second-order formula cannot pass
    assert kl_err <= klb["bound"], (stats[3].item(), klb)
    k.close()


def test_adam_step_vs_torch():
    pol = _policy()
    k = MlpKernels(256, DEV)
    n = k.num_params
    g = torch.Generator(device=DEV).manual_seed(5)
    params = pol.flat.clone()
    ref_p = torch.nn.Parameter(pol.flat.clone())
    opt = torch.optim.Adam([ref_p], lr=6e-6, eps=1e-5)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    for step in range(1, 6):
        grad = torch.randn(n, device=DEV, generator=g) * (0.01 if step % 2 else 1e-4)  # with and without clipping
        ref_p.grad = grad.clone()
        torch.nn.utils.clip_grad_norm_([ref_p], 0.5)
        opt.step()
        k.adam_step(params, grad, m, v, lr=6e-6, eps=1e-5, max_grad_norm=0.5, step=step)
        assert torch.allclose(params, ref_p.data, rtol=0, atol=6e-8), (params - ref_p.data).abs().max()  # 1 ulp at |p| ~ 0.5; the update itself is ~6e-6
    # the kernel-format weights follow the flat vector: forward uses the updated parameters
    pol.flat.copy_(params)
    obs = torch.rand((256, 56), device=DEV, generator=g)
    mean, value = k.mean_value(obs)
    rm, rv = P.mlp_forward(pol.views, obs)
    assert torch.allclose(mean, rm, rtol=1e-4, atol=2e-5) and torch.allclose(value, rv, rtol=1e-4, atol=2e-5)
    k.close()


def test_gae_scan_vs_sb3_formula():
    import ctypes as C
    from rl_brain_trainer_amd import native

    T, N = 96, 1000
    g = torch.Generator(device=DEV).manual_seed(2)
    rew = torch.randn((T, N), device=DEV, generator=g)
    val = torch.randn((T, N), device=DEV, generator=g)
    done = (torch.rand((T, N), device=DEV, generator=g) < 0.05).to(torch.uint8) * 2
    done[10] |= 1
    last = torch.randn(N, device=DEV, generator=g)
    adv = torch.empty((T, N), device=DEV)
    ret = torch.empty((T, N), device=DEV)
    L = native.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    native.check(L.kp1_gae_scan(0, p(rew), p(val), p(done), p(last), 0.995, 0.95, p(adv), p(ret), T, N, None))
    # SB3 RolloutBuffer.compute_returns_and_advantage in numpy
    r, v, d, lv = rew.cpu().numpy(), val.cpu().numpy(), (done.cpu().numpy() & 3) != 0, last.cpu().numpy()
    ref = np.zeros((T, N), dtype=np.float32)
    lg = np.zeros(N, dtype=np.float32)
    for t in reversed(range(T)):
        nv = lv if t == T - 1 else v[t + 1]
        nonterm = 1.0 - d[t].astype(np.float32)
        delta = r[t] + np.float32(0.995) * nv * nonterm - v[t]
        lg = delta + np.float32(0.995 * 0.95) * nonterm * lg
        ref[t] = lg
    assert np.allclose(adv.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    assert np.allclose(ret.cpu().numpy(), ref + v, rtol=1e-5, atol=1e-5)


def test_device_curriculum_matches_golden_tracker():
    import json
    from conftest import GOLDEN

    cases = json.loads((GOLDEN / "curriculum_tracker.json").read_text())["cases"]
    for case in cases:
        cur = PointCurriculum(success_rate_threshold=case["threshold"], window_episodes=case["window"],
                              min_episodes_per_stage=case["min_episodes"], max_stage_index=case["n_stages"] - 1, device=0)
        seq = np.array(case["successes"], dtype=np.uint8)
        # feed in VecEnv-sized slices with idle envs in between (done bit 2 = truncated, bit 4 = success)
        n = 96
        stages = []
        for s in range(0, len(seq), 7):
            chunk = seq[s:s + 7]
            dones = np.zeros(n, dtype=np.uint8)
            pos = np.sort(np.random.default_rng(s).choice(n, size=len(chunk), replace=False))
            dones[pos] = 2 | (chunk << 2)
            cur.observe(torch.tensor(dones, device=DEV), n)
            stages.append(cur.read().stage_index)
        summ = cur.summary()
        assert [h["to_stage_index"] for h in summ["history"]] == list(range(1, len(case["promoted_at"]) + 1))
        assert [h["trigger_success_rate"] for h in summ["history"]] == case["trigger_rates"]
        assert summ["stage_index"] == case["stage_after"][-1]
        # stage after each slice equals the reference tracker's stage after the last episode of that slice
        ends = [min(s + 7, len(seq)) - 1 for s in range(0, len(seq), 7)]
        assert stages == [case["stage_after"][e] for e in ends]
        cur.close()


@pytest.mark.parametrize("window,min_eps,max_stage,n_big", [(64, 100, 11, 4096), (20, 48, 5, 8192), (48, 300, 2, 5000), (1000, 1100, 3, 4096)])
def test_device_curriculum_parallel_path_equals_serial_replay(window, min_eps, max_stage, n_big):
    """The tracker's whole-wave path (>= 192 finished episodes in a block of 4096 envs: prefix counts, first promotion by wave-min, closed-form
    window update) against its serial lane-0 replay, which the golden traces pin: the same episode stream fed as big VecEnv steps (every env
    finishes: 4096 / 8192 / 5000 with idle envs) and as 64-env steps must leave the same stage, episode count, window (length, head, live
    entries) and promotion history (from / to / trigger rate).  Success rates drift up and down so that promotions fall inside, at the start and
    at the end of blocks, several per block, and stop at the last stage."""
    g = np.random.default_rng(window + n_big)
    total = 60000
    phase = np.sin(np.arange(total) / 1500.0) * 0.25 + 0.7
    seq = (g.random(total) < phase).astype(np.uint8)
    kw = dict(success_rate_threshold=0.75, window_episodes=window, min_episodes_per_stage=min_eps, max_stage_index=max_stage, initial_stage_index=0, device=0)
    big, small = PointCurriculum(**kw), PointCurriculum(**kw)
    used = 0
    while used + n_big <= total:
        dones = np.zeros(n_big, dtype=np.uint8)
        k = n_big if n_big != 5000 else 4300                    # 5000 envs, 4300 of them finish (idle envs in between; second block ragged)
        pos = np.arange(n_big) if k == n_big else np.sort(g.choice(n_big, size=k, replace=False))
        dones[pos] = 2 | (seq[used:used + k] << 2)
        big.observe(torch.tensor(dones, device=DEV), n_big)
        for s0 in range(used, used + k, 64):
            chunk = seq[s0:min(s0 + 64, used + k)]
            d = np.zeros(64, dtype=np.uint8)
            d[:len(chunk)] = 2 | (chunk << 2)
            small.observe(torch.tensor(d, device=DEV), 64)
        used += k
        a, b = big.read(), small.read()
        assert (a.stage_index, a.stage_episode_count, a.ring_len, a.ring_head, a.n_events) == (b.stage_index, b.stage_episode_count, b.ring_len, b.ring_head, b.n_events), used
        live = [(a.ring_head + j) % window for j in range(a.ring_len)]
        assert [a.ring[j] for j in live] == [b.ring[j] for j in live], used
    a, b = big.read(), small.read()
    assert a.n_events >= 1 and (a.stage_index == max_stage or a.n_events >= 2)
    for k in range(min(a.n_events, 64)):
        ea, eb = a.events[k], b.events[k]
        assert (ea.from_stage, ea.to_stage, ea.trigger_success_rate) == (eb.from_stage, eb.to_stage, eb.trigger_success_rate), k
    big.close()
    small.close()


def test_placement_self_check_reports_the_launch_shape():
    """kp1_mlp_placement_check: the probe has the training tile's launch shape (two workgroups of 8192 / 32 tiles x 2 nets per CU), every workgroup
    is resident at once, and the report is internally consistent.  What the placement IS on the box is reported by bench.py, not asserted here: the
    assumptions are speed assumptions."""
    from rl_brain_trainer_amd.mlp import MlpKernels

    mlp = MlpKernels(256, torch.device(DEV), max_batch=8192)
    rep = mlp.placement_check(8192)
    assert rep["workgroups"] == 512 and rep["all_resident"]
    assert 0 < rep["compute_units_used"] <= rep["compute_units"]
    assert rep["second_tile_pairs"] == 512 - rep["compute_units"] and 0 <= rep["second_tile_on_same_cu"] <= rep["second_tile_pairs"]
    assert 0 <= rep["on_xcd_of_block_index_mod_8"] <= 512 and 1 <= rep["xcds_among_first_8_blocks"] <= 8
    small = mlp.placement_check(512)
    assert small["workgroups"] == 32 and small["second_tile_pairs"] == 0
    mlp.close()


def test_keyed_permutation_is_a_permutation_and_mixes():
    """kp1_random_permutation (the minibatch shuffle above 2^17 samples): a bijection of [0, n) for any n (cycle walking below the next
    power of two), different keys give different permutations, and consecutive outputs -- one minibatch is a run of them -- look like
    uniform draws: occupancy of 64 equal bins by the first 8192 outputs within chi-square bounds, no lag-1 correlation."""
    import ctypes as C

    from rl_brain_trainer_amd import native

    L = native.load()
    rng = np.random.default_rng(5)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def draw(n, keys):
        out = torch.empty(n, dtype=torch.int64, device=DEV)
        k = np.asarray(keys, dtype=np.uint32)
        native.check(L.kp1_random_permutation(0, n, k.ctypes.data_as(C.c_void_p), C.c_void_p(out.data_ptr()), stream))
        return out

    def host_restatement(n, keys):
        """the construction include/kp1_ppo.h documents: four rounds of (odd multiply + add, xorshift by bits // 2) modulo 2^bits, cycle-walked"""
        bits = 1
        while (1 << bits) < n:
            bits += 1
        mask, sh = np.uint64((1 << bits) - 1), np.uint64(bits // 2 if bits > 1 else 1)
        mul = [np.uint64(int(k) | 1) for k in keys[:4]]
        add = [np.uint64(int(k)) for k in keys[4:]]
        out = np.empty(n, dtype=np.int64)
        todo, cur = np.arange(n), np.arange(n, dtype=np.uint64)
        while todo.size:
            for r in range(4):
                cur = ((cur * mul[r] + add[r]) & np.uint64(0xFFFFFFFF)) & mask
                cur ^= cur >> sh
            ok = cur < n
            out[todo[ok]] = cur[ok].astype(np.int64)
            todo, cur = todo[~ok], cur[~ok]
        return out

    for n in (1, 2, 3, 5, 1000, 1 << 17, 524288, 524289, 1_000_003):
        keys = rng.integers(0, 1 << 32, size=8, dtype=np.uint64)
        p = draw(n, keys)
        assert torch.equal(torch.sort(p).values, torch.arange(n, device=DEV)), n
        assert np.array_equal(p.cpu().numpy(), host_restatement(n, keys)), n
        if n >= 1000:
            q = draw(n, rng.integers(0, 1 << 32, size=8, dtype=np.uint64))
            assert (p == q).float().mean().item() < 0.01                      # another key, another permutation
            assert (p == torch.arange(n, device=DEV)).float().mean().item() < 0.01
    n = 524288
    for trial in range(8):
        p = draw(n, rng.integers(0, 1 << 32, size=8, dtype=np.uint64)).cpu().numpy()
        head = p[:8192]
        counts = np.bincount(head * 64 // n, minlength=64)
        chi2 = ((counts - 128.0) ** 2 / 128.0).sum()                           # 63 degrees of freedom: mean 63, sd 11.2
        assert chi2 < 63 + 6 * 11.3, (trial, chi2)
        x = p.astype(np.float64) / n - 0.5
        assert abs(np.mean(x[:-1] * x[1:]) * 12.0) < 0.01, trial               # lag-1 correlation of consecutive outputs
        assert abs(np.mean(x * (np.arange(n) / n - 0.5)) * 12.0) < 0.01, trial  # and none with the input index


def test_adv_minibatch_sums_vs_torch():
    """per-epoch advantage statistics: every minibatch's (sum, sum^2, count) in one launch, ragged last minibatch included"""
    import ctypes as C

    from rl_brain_trainer_amd import native

    L = native.load()
    g = torch.Generator(device=DEV).manual_seed(11)
    total, mb = 10000, 3000
    adv = torch.randn(total, device=DEV, generator=g) * 2 + 0.3
    perm = torch.randperm(total, device=DEV, generator=g)
    n_mb = (total + mb - 1) // mb
    out = torch.zeros((n_mb, 3), dtype=torch.float64, device=DEV)
    native.check(L.kp1_adv_minibatch_sums(0, C.c_void_p(adv.data_ptr()), C.c_void_p(perm.data_ptr()), total, mb, C.c_void_p(out.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for b in range(n_mb):
        sel = adv[perm[b * mb:(b + 1) * mb]].double()
        assert out[b, 2].item() == sel.numel()
        assert abs(out[b, 0].item() - sel.sum().item()) <= 1e-9 * sel.abs().sum().item()
        assert abs(out[b, 1].item() - (sel * sel).sum().item()) <= 1e-9 * (sel * sel).sum().item()
    # (sum, sum^2, count) -> (mean, 1 / (std + 1e-8)): one launch against SB3's tensor expression (torch.std is unbiased)
    stats = torch.zeros((n_mb, 2), dtype=torch.float32, device=DEV)
    native.check(L.kp1_adv_minibatch_stats(0, C.c_void_p(out.data_ptr()), n_mb, C.c_void_p(stats.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for b in range(n_mb):
        sel = adv[perm[b * mb:(b + 1) * mb]]
        assert abs(stats[b, 0].item() - sel.mean().item()) <= 1e-6
        assert abs(stats[b, 1].item() - 1.0 / (sel.std().item() + 1e-8)) <= 1e-5 * stats[b, 1].item()
    # a one-sample minibatch: variance 0 -> 1 / 1e-8, as (x - mean) / (0 + 1e-8) needs
    one = torch.tensor([[2.5, 6.25, 1.0]], dtype=torch.float64, device=DEV)
    st1 = torch.zeros((1, 2), dtype=torch.float32, device=DEV)
    native.check(L.kp1_adv_minibatch_stats(0, C.c_void_p(one.data_ptr()), 1, C.c_void_p(st1.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert st1[0, 0].item() == 2.5 and st1[0, 1].item() == pytest.approx(1e8, rel=1e-6)


def test_compacted_truncation_bootstrap_matches_dense_path():
    """collect_rollouts' time-limit bootstrap: critic on the truncated steps only (fixed-size index list) vs critic on all T * N
    terminal observations + kp1_bootstrap_truncated."""
    from conftest import load_golden_config
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    cfg = load_golden_config("workspace_expansion_bigtrain")
    env = ArmKinematicVecEnv(cfg, 512, seed=3)
    env.set_curriculum_stage(5)
    ppo = P.PPO(env, P.PPOConfig(n_steps=128, batch_size=4096, n_epochs=1, hidden=256, seed=3), backend="hip", use_graphs=False)
    ppo.collect_rollouts()                      # real done / terminal_obs buffers (96-step episodes: every env truncates once or twice)
    trunc = ((ppo.done_buf & 3) == 2)
    assert 512 <= int(trunc.sum()) <= 1024
    g = torch.Generator(device=DEV).manual_seed(9)
    raw = torch.randn(ppo.rew_buf.shape, device=DEV, generator=g)
    ppo.rew_buf.copy_(raw)
    ppo._bootstrap_truncated(dense=True)
    dense = ppo.rew_buf.clone()
    ppo.rew_buf.copy_(raw)
    ppo._bootstrap_truncated()
    assert torch.equal((ppo.rew_buf != raw), trunc)
    assert torch.allclose(ppo.rew_buf, dense, rtol=0, atol=1e-6)
    env.close()


def test_layerwise_weight_copies_follow_adam_after_option_switch():
    """While the fused path is selected kp1_mlp_adam_step refreshes only the fragment-major weight copies; switching to the layer-wise
    kernels must first bring their k-slab copies up to date (KP1_MLP_OPT_FUSED, kp1_mlp_set_option)."""
    pol = _policy()
    k = MlpKernels(256, DEV, max_batch=4096)
    k.pack(pol.flat)
    g = torch.Generator(device=DEV).manual_seed(2)
    m = torch.zeros_like(pol.flat)
    v = torch.zeros_like(pol.flat)
    for step in (1, 2, 3):
        grad = 1e-2 * torch.randn(pol.flat.numel(), device=DEV, generator=g)
        k.adam_step(pol.flat, grad, m, v, lr=1e-2, eps=1e-5, max_grad_norm=0.5, step=step)
    obs = torch.rand((512, 56), device=DEV, generator=g) * 2 - 1
    ref_mean, ref_value = P.mlp_forward(pol.views, obs)
    for fused in (True, False, True):
        k.set_fused(fused)
        mean, value = k.mean_value(obs)
        assert torch.allclose(mean, ref_mean, rtol=1e-4, atol=2e-5) and torch.allclose(value, ref_value, rtol=1e-4, atol=2e-5), fused
    k.close()


def test_ppo_optimiser_step_matches_cpu_oracle():
    """One full optimiser step (MFMA loss / gradient, clip_grad_norm_, Adam, weight repack) against oracle/ppo_oracle.py, the CPU
    restatement of SB3's PPO.train inner loop, from the same parameters on the same minibatch.  fp32 both sides; tolerance = the
    summation-order differences of the gradient (2e-4 of its scale) carried through one Adam step."""
    from oracle import ppo_oracle as po

    cpu = po.ActorCriticCPU(56, 256, 7, seed=4)
    with torch.no_grad():
        cpu.log_std.copy_(torch.tensor([-0.3, 0.1, -0.5, 0.0, 0.2, -0.1, -0.7]))
        cpu.action_head.weight.mul_(10.0)
    pol = P.ActorCritic(256, DEV, seed=0)
    pol.flat.copy_(po.flat_params_sb3_order(cpu).to(DEV))
    k = MlpKernels(256, DEV, max_batch=8192)
    k.pack(pol.flat)
    g = torch.Generator().manual_seed(12)
    n = 4096
    obs = torch.rand((n, 56), generator=g) * 2 - 1
    with torch.no_grad():
        mean, values = cpu(obs)
    act = mean + torch.exp(cpu.log_std.detach()) * torch.randn((n, 7), generator=g)
    old = cpu.log_prob(act, mean + 0.05 * torch.randn((n, 7), generator=g)).detach()
    adv = torch.randn(n, generator=g) * 2 + 0.3
    ret = values + torch.randn(n, generator=g)
    lr, clip, ent, vf = 1e-3, 0.1, 3e-4, 0.5
    opt = torch.optim.Adam(cpu.parameters(), lr=lr, eps=1e-5)
    before = po.flat_params_sb3_order(cpu).clone()
    terms = po.train_minibatch(cpu, opt, obs, act, old, adv, ret, clip_range=clip, ent_coef=ent, vf_coef=vf, max_grad_norm=0.5)
    after = po.flat_params_sb3_order(cpu)

    d = lambda t: t.to(DEV).contiguous()   # noqa: E731
    grad = torch.empty(k.num_params, device=DEV)
    stats = torch.zeros(4, device=DEV)
    m, v = torch.zeros_like(pol.flat), torch.zeros_like(pol.flat)
    k.loss_grad(d(obs), None, n, d(act), d(old), d(adv), d(ret), clip_range=clip, ent_coef=ent, vf_coef=vf, inv_count=1.0 / n, grad_out=grad, stats_out=stats)
    k.adam_step(pol.flat, grad, m, v, lr=lr, eps=1e-5, max_grad_norm=0.5, step=1, fused_norm=True)
    assert abs(stats[0].item() - terms["policy_loss"]) <= 1e-4 * (1 + abs(terms["policy_loss"]))
    assert abs(stats[1].item() - terms["value_loss"]) <= 1e-4 * (1 + abs(terms["value_loss"]))
    delta_ref = (after - before).to(DEV)
    delta = pol.flat - before.to(DEV)
    # first Adam step: delta = -lr * g / (|g| + eps) -- about lr * sign(g) wherever |g| >> eps = 1e-5, and sensitive to the last bits of g
    # where |g| ~ eps (d delta / d g = lr * eps / (|g| + eps)^2): bound the bulk tightly and the eps-sized gradients loosely
    err = (delta - delta_ref).abs()
    assert torch.quantile(err, 0.99).item() <= 2e-2 * lr and err.max().item() <= 0.3 * lr, (torch.quantile(err, 0.99).item(), err.max().item())
    big = delta_ref.abs() > 0.5 * lr
    assert big.float().mean() > 0.5 and torch.equal(torch.sign(delta[big]), torch.sign(delta_ref[big]))
    mean2, value2 = k.mean_value(d(obs))
    with torch.no_grad():
        rm, rv = cpu(obs)
    assert torch.allclose(mean2.cpu(), rm, rtol=1e-3, atol=2e-4) and torch.allclose(value2.cpu(), rv, rtol=1e-3, atol=2e-4)
    k.close()


@pytest.mark.parametrize("hidden", [128, 64])
@pytest.mark.parametrize("obs_dim", [56, 80])
def test_hidden128_layerwise_path(obs_dim, hidden):
    """net_arch 2x128 and 2x64 -- SB3's default, the width the reference trains (train_workspace_expansion.py:199, no policy_kwargs) and its
    checkpoints hold -- run through the layer-wise MFMA kernels (2x64 on a zero-padded 128-wide layout): forward, loss / gradient and the
    optimiser step against torch, both observation widths."""
    D, W = obs_dim, (64 if obs_dim <= 64 else 128)
    pol = _policy(hidden=hidden, scale_heads=False, obs_dim=D)
    k = MlpKernels(hidden, DEV, max_batch=8192, obs_dim=D)
    assert k.num_params == pol.flat.numel()
    k.pack(pol.flat)
    g = torch.Generator(device=DEV).manual_seed(21)
    total, n = 9000, 5000
    obs = torch.zeros((total, W), device=DEV)
    obs[:, :D] = torch.rand((total, D), device=DEV, generator=g) * 2 - 1
    mean, value = k.mean_value(obs[:3000].contiguous())
    with torch.no_grad():
        m0, v0 = P.mlp_forward(pol.views, obs[:, :D].contiguous())
    assert torch.allclose(mean, m0[:3000], rtol=1e-4, atol=2e-5) and torch.allclose(value, v0[:3000], rtol=1e-4, atol=2e-5)
    act = m0 + torch.exp(pol.views["log_std"]) * torch.randn((total, 7), device=DEV, generator=g)
    old_logp = P.gaussian_log_prob(act, m0 + 0.05 * torch.randn((total, 7), device=DEV, generator=g), pol.views["log_std"])
    adv = torch.randn(total, device=DEV, generator=g) * 2 + 0.3
    ret = v0 + torch.randn(total, device=DEV, generator=g)
    idx = torch.randperm(total, device=DEV, generator=g)[:n]
    grad = torch.empty(k.num_params, device=DEV)
    stats = torch.zeros(4, device=DEV)
    k.loss_grad(obs, idx, n, act, old_logp, adv, ret, clip_range=0.1, ent_coef=3e-4, vf_coef=0.5, inv_count=1.0 / n, grad_out=grad, stats_out=stats)
    a = adv[idx]
    a = (a - a.mean()) / (a.std() + 1e-8)
    ref = P.ppo_loss_and_grad_torch(pol.flat, pol.spec, obs[idx, :D], act[idx], old_logp[idx], a, ret[idx], clip_range=0.1, ent_coef=3e-4, vf_coef=0.5)
    off = 0
    for name, shape in pol.spec:
        cnt = math.prod(shape)
        gk, gr = grad[off:off + cnt], ref[off:off + cnt]
        scale = gr.abs().max().item() + 1e-12
        assert (gk - gr).abs().max().item() <= 2e-4 * scale + 1e-7, name
        off += cnt
    # optimiser step + repack keep the layer-wise weight copies current
    m, v = torch.zeros_like(pol.flat), torch.zeros_like(pol.flat)
    before = pol.flat.clone()
    k.adam_step(pol.flat, grad, m, v, lr=1e-3, eps=1e-5, max_grad_norm=0.5, step=1)
    # clip_grad_norm_(0.5) + Adam step 1 in torch on the reference gradient: the padded units of the 2x64 layout must not leak into the norm
    gref = ref * torch.clamp(0.5 / (torch.linalg.vector_norm(ref) + 1e-6), max=1.0)
    expect = before - 1e-3 * (0.1 * gref / (1 - 0.9)) / ((0.001 * gref * gref).sqrt() / math.sqrt(1 - 0.999) + 1e-5)
    big = gref.abs() > 1e-3 * gref.abs().max()          # where g ~ 0 Adam's sign(g) step amplifies rounding noise
    assert (pol.flat - expect)[big].abs().max().item() <= 2e-5
    mean2, _ = k.mean_value(obs[:512].contiguous())
    m2, _ = P.mlp_forward(pol.views, obs[:512, :D].contiguous())
    assert torch.allclose(mean2, m2, rtol=1e-4, atol=2e-5)
    k.close()


def test_reference_width_policy_trains_on_hip_backend():
    """PPO with SB3's default 2x64 policy (PPOConfig.hidden default) uses the HIP backend end to end: rollout, update, checkpoint round trip
    through InferencePolicy -- no torch backend in the product path."""
    from conftest import load_golden_config
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    env = ArmKinematicVecEnv(load_golden_config("workspace_expansion_bigtrain"), 256, seed=806)
    env.set_curriculum_stage(5)
    ppo = P.PPO(env, P.PPOConfig(n_steps=32, batch_size=2048, n_epochs=2, learning_rate=3e-4, seed=1), backend="hip")
    assert ppo.cfg.hidden == 64 and ppo._mlp is not None
    before = ppo.policy.flat.clone()
    for _ in range(3):
        ppo.collect_rollouts()
        ppo.train()
    torch.cuda.synchronize()
    assert torch.isfinite(ppo.policy.flat).all() and (ppo.policy.flat != before).any()
    pol = P.InferencePolicy(ppo.policy.state_dict())
    obs = ppo.obs_buf[0, :64].contiguous()
    ref, _ = P.mlp_forward(ppo.policy.views, obs[:, :56].contiguous())
    assert torch.allclose(pol.predict(obs), ref.clamp(-1, 1), rtol=1e-4, atol=2e-5)
    env.close()


@pytest.mark.parametrize("mode", ["raw", "given"])
def test_loss_grad_advantage_modes(mode):
    """normalize_advantage=False (raw advantages) and externally supplied (mean, 1/std) -- the data-parallel path's global statistics --
    against torch autograd with the same advantages; the default per-minibatch normalisation is covered above."""
    pol = _policy(scale_heads=False)
    k = MlpKernels(256, DEV, max_batch=4096)
    k.pack(pol.flat)
    g = torch.Generator(device=DEV).manual_seed(31)
    n = 3000
    obs = torch.zeros((n, 64), device=DEV)
    obs[:, :56] = torch.rand((n, 56), device=DEV, generator=g) * 2 - 1
    with torch.no_grad():
        m0, v0 = P.mlp_forward(pol.views, obs[:, :56].contiguous())
    act = m0 + torch.exp(pol.views["log_std"]) * torch.randn((n, 7), device=DEV, generator=g)
    old_logp = P.gaussian_log_prob(act, m0 + 0.05 * torch.randn((n, 7), device=DEV, generator=g), pol.views["log_std"])
    adv = torch.randn(n, device=DEV, generator=g) * 0.7 + 0.2
    ret = v0 + torch.randn(n, device=DEV, generator=g)
    grad = torch.empty(k.num_params, device=DEV)
    if mode == "raw":
        k.loss_grad(obs, None, n, act, old_logp, adv, ret, clip_range=0.2, ent_coef=1e-3, vf_coef=0.5, inv_count=1.0 / n, grad_out=grad, stats_out=None, normalize=False)
        a = adv
    else:
        stats = torch.tensor([0.37, 1.9], device=DEV)
        k.loss_grad(obs, None, n, act, old_logp, adv, ret, clip_range=0.2, ent_coef=1e-3, vf_coef=0.5, inv_count=1.0 / n, grad_out=grad, stats_out=None, adv_stats=stats)
        a = (adv - 0.37) * 1.9
    ref = P.ppo_loss_and_grad_torch(pol.flat, pol.spec, obs[:, :56], act, old_logp, a, ret, clip_range=0.2, ent_coef=1e-3, vf_coef=0.5)
    off = 0
    for name, shape in pol.spec:
        cnt = math.prod(shape)
        gk, gr = grad[off:off + cnt], ref[off:off + cnt]
        scale = gr.abs().max().item() + 1e-12
        assert (gk - gr).abs().max().item() <= 2e-4 * scale + 1e-7, (mode, name)
        off += cnt
    k.close()


@pytest.mark.parametrize("cfg_name,stage,n_envs,n_steps", [("workspace_expansion_bigtrain", 5, 1000, 100),
                                                           ("dock_workspace_handoff_noop_ft_12env_raw", 0, 320, 80)])
def test_fused_policy_env_step_equals_two_launches(cfg_name, stage, n_envs, n_steps, monkeypatch):
    """kp1_mlp_forward_env_step (policy forward, sampling and the env step of a 32-row tile in ONE launch: mlp_tile_kernel<false, 2, ENV>)
    against kp1_mlp_forward + kp1_step on identical seeds: a whole rollout with auto-resets -- observations, actions, log-probs, values,
    rewards, done bytes, terminal observations, advantages, every env state field and all PCG64 streams bit for bit.  1000 / 320 envs: the
    last tile is ragged (rows >= n are masked out of the env step)."""
    cfg = load_golden_config(cfg_name)
    out = {}
    for form in ("1", "0"):
        monkeypatch.setenv("KP1_FUSED_ROLLOUT", form)
        env = ArmKinematicVecEnv(cfg, n_envs, seed=21, real="f32")
        env.set_curriculum_stage(stage)
        cur = PointCurriculum(success_rate_threshold=0.0, window_episodes=8, min_episodes_per_stage=8, max_stage_index=11, initial_stage_index=stage) \
            if cfg.c.curriculum_enabled else None
        ppo = P.PPO(env, P.PPOConfig(n_steps=n_steps, batch_size=n_envs * n_steps // 4, n_epochs=1, hidden=256, learning_rate=3e-4, seed=5), curriculum=cur,
                    backend="hip")
        assert ppo._fused_env_step == (form == "1") and ppo.use_graphs
        bufs = []
        for _ in range(2):                       # the first rollout captures (warm-up between snapshot and restore), the second replays
            ppo.collect_rollouts()
            torch.cuda.synchronize()
            bufs.append({k: getattr(ppo, k).clone() for k in ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "term_obs_buf", "adv_buf")})
        info = {k: v.clone() for k, v in env.info().items()}
        out[form] = (bufs, info, env.rng_state(), None if cur is None else cur.read().stage_index)
        if cur is not None:
            cur.close()
        env.close()
    (b1, i1, r1, s1), (b0, i0, r0, s0) = out["1"], out["0"]
    assert int((b0[1]["done_buf"] & 3 != 0).sum()) + int((b0[0]["done_buf"] & 3 != 0).sum()) >= n_envs      # auto-resets happened
    for x, y in zip(b1, b0):
        for k in x:
            assert torch.equal(x[k], y[k]), k
    for k in i0:
        assert torch.equal(i1[k], i0[k]), k
    assert np.array_equal(r1, r0) and s1 == s0
