"""Shared by test_row_attribution_gpu.py, test_row_attribution_cpu.py and the approx_kl assertions of the loss tests: minibatches in which
every row contributes exactly nothing to the PPO loss except a small set S of spike rows, placed where the kernels change tile, stage or
chunk; the fp64 references over S alone; and the bound of the approx_kl comparison.  Everything here is plain torch on the CPU (the GPU
module moves the inputs over), in the idiom of tests/mlp_handle_state.py."""
from __future__ import annotations

import torch

import mlp_handle_state as S
from rl_brain_trainer_amd import ppo as P

N, MAX_BATCH = 2065, 2176
CLIP_RANGE, VF_COEF, LOSS_WEIGHT = 0.2, 0.5, 0.5
ANCHOR_KINDS = [kd for kd in S.KINDS if kd[0] != 256]           # kp1_mlp_anchor_loss_grad runs on the Hp = 128 layer-wise kernels only
ACTOR = ("mlp_extractor.policy_net.", "action_net.")            # the six tensors the teacher anchor reaches
POLICY = ("log_std",) + ACTOR                                   # the tensors of the policy-side run; every other tensor is the value side's


# ------------------------------------------------------------------------------------------------ where the kernels change unit at n rows
def tn_chunk_rows(n: int, tiles: int) -> int:
    """kp1_mlp.hip tn_chunk_rows: rows of the batch one weight-gradient workgroup of the layer-wise path reduces"""
    chunks = min(max((256 + tiles - 1) // tiles, 1), 64)
    rows = ((n + chunks - 1) // chunks + 63) // 64 * 64
    return max(rows, 64)


def units(kind, n: int, anchor: bool = False) -> dict[str, int]:
    """name -> rows per unit of every batch partition kp1_mlp_loss_grad (anchor: kp1_mlp_anchor_loss_grad) launches at n rows, restated
    from the launch code of kp1_mlp.hip"""
    hidden, _, path = kind
    if path == "fused":            # mlp_tile_kernel + gemm_tn_frag_kernel (kp1_mlp_loss_grad, `if (fused)`)
        groups = (n + 31) // 32 * 4                               # t.groups: 8-row fragment groups of whole FU_BM = 32-row tiles
        up8 = lambda v: (v + 7) // 8 * 8                          # noqa: E731
        cg2, cg1 = up8((groups + 7) // 8), up8((groups + 15) // 16)   # TN_SPLIT2 = 8, TN_SPLIT1 = 16
        return {"fragment group": 8, "row tile (FU_BM)": 32, "dW2 chunk (cg2)": 8 * cg2, "dW1 chunk (cg1)": 8 * cg1}
    hp = 256 if hidden == 256 else 128                            # 2x64 runs on the zero-padded 128-wide layout
    if anchor:                     # both weight gradients on tn_chunk_rows(n, 2)
        c2 = c1 = tn_chunk_rows(n, 2)
    else:
        c2, c1 = tn_chunk_rows(n, (hp // 128) ** 2 * 2), tn_chunk_rows(n, (hp // 128) * 2)
    return {"head tile (HEAD_ROWS)": 32, "row tile of gemm_nt / stage of gemm_tn": 64, "dW2 chunk": c2, "dW1 chunk": c1}


def boundaries(kind, n: int, anchor: bool = False) -> dict[str, tuple[int, int]]:
    """name -> (first row of the second unit, first row of the last unit)"""
    return {name: (rows, (n - 1) // rows * rows) for name, rows in units(kind, n, anchor).items()}


# Spike positions (batch positions, not buffer rows).  From the launch code at n = 2065 (units() above restates it):
#   fused 2x256    65 row tiles of FU_BM = 32 (the last holds 17 rows: 2048 .. 2064) = 260 fragment groups of 8 rows, the last of them holding
#                  row 2064 alone; cg2 = up8(ceil(260 / 8)) = 40 groups = 320 rows -> 7 dW2 chunks, the last from row 1920;
#                  cg1 = up8(ceil(260 / 16)) = 24 groups = 192 rows -> 11 dW1 chunks, the last from row 1920.  A chunk is reduced in 64-row
#                  stages, so a 320-row chunk runs the double-buffered stage loop five times and a 192-row chunk three times
#   layer 2x256    head tiles of HEAD_ROWS = 32, gemm_nt row tiles of 64 (33 of them: below launch_nt's wide-tile switch); dW2:
#                  tn_chunk_rows(2065, 8) = 128 rows -> 17 chunks of two stages, the last from row 2048 with 17 rows; dW1:
#                  tn_chunk_rows(2065, 4) = 64 rows -> 33 chunks
#   layer 2x128, 2x64 and K = 3 populations (Hp = 128)   the same head and row tiles; dW2 tn_chunk_rows(2065, 2) = 64 rows and dW1
#                  tn_chunk_rows(2065, 2) = 64 rows -> 33 chunks each, the last from row 2048; the anchor step uses tn_chunk_rows(n, 2) for both
# Hence: the first and the last row (0, 2064); the row before and the row at the first boundary of every unit (8, 32, 64, 128, 192, 320) and at
# the second dW1 boundary of the fused path (384); the same around the start of the last unit (1920, 2048, and 2064, where the last fragment
# group starts); and three interior rows from a seeded draw.
BOUNDARY_POSITIONS = [0, 7, 8, 31, 32, 63, 64, 127, 128, 191, 192, 319, 320, 383, 384, 1919, 1920, 2047, 2048, 2063, 2064]


def _interior(count: int = 3, seed: int = 2065) -> list[int]:
    perm = torch.randperm(N, generator=torch.Generator(device="cpu").manual_seed(seed)).tolist()
    return sorted([p for p in perm if all(abs(p - b) > 8 for b in BOUNDARY_POSITIONS)][:count])


POSITIONS = sorted(BOUNDARY_POSITIONS + _interior())
NS = len(POSITIONS)


# ------------------------------------------------------------------------------------------------ the minibatch
def _signed(shape, lo: float, hi: float, g) -> torch.Tensor:
    """random sign x uniform [lo, hi]"""
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1) * (lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64))


def build(hidden: int, obs_dim: int, *, gather: bool, K: int = 1) -> dict:
    """K replicas (K = 1: a single handle), replica r owning buffer rows [r * 2176, (r + 1) * 2176): its policy, its selection idx[r] of 2065 of
    them (gather) or their first 2065 (prefix form, K = 1), and for every buffer row spike-sized values of its own.  Which rows are spikes is
    decided by batch position: buffer row idx[r][p] for p in POSITIONS.  The other selected rows are silenced by policy_side / value_side /
    anchor_side; rows outside the selection keep their spike-sized values, so a kernel that reads one shows."""
    D, W, total = obs_dim, S.pitch(obs_dim), K * MAX_BATCH
    g = torch.Generator(device="cpu").manual_seed(100000 + 1000 * K + 10 * hidden + obs_dim + int(gather))
    pols = [S.policy(hidden, obs_dim, seed=3 + 10 * r) for r in range(K)]
    spec = pols[0].spec
    obs = torch.zeros((total, W))
    obs[:, :D] = torch.rand((total, D), generator=g) * 2 - 1
    noise = torch.randn((total, 7), generator=g, dtype=torch.float64)
    mean64, value64, logp64 = torch.empty((total, 7), dtype=torch.float64), torch.empty(total, dtype=torch.float64), torch.empty(total, dtype=torch.float64)
    act = torch.empty((total, 7))
    for r, pol in enumerate(pols):
        rows = slice(r * MAX_BATCH, (r + 1) * MAX_BATCH)
        Pv = S.views_of(pol.flat.double(), spec)
        mean64[rows], value64[rows] = P.mlp_forward(Pv, obs[rows, :D].double())
        act[rows] = (mean64[rows] + torch.exp(Pv["log_std"]) * noise[rows]).float()
        logp64[rows] = P.gaussian_log_prob(act[rows].double(), mean64[rows], Pv["log_std"])
    idx = torch.stack([r * MAX_BATCH + (S.selection(MAX_BATCH, N, 600 + r) if gather else torch.arange(N)) for r in range(K)]).contiguous()
    pos = torch.tensor(POSITIONS)
    spike_rows = idx[:, pos].contiguous()                                         # [K][NS] buffer rows
    is_spike = torch.zeros(total, dtype=torch.bool)
    is_spike[spike_rows.reshape(-1)] = True
    silent = torch.zeros(total, dtype=torch.bool)
    silent[idx.reshape(-1)] = True
    silent &= ~is_spike
    # spike rows: inside the clip range (|log ratio| <= 0.1 < log 1.2 and < -log 0.8), so the row carries policy gradient; the others spread wider
    spread = torch.where(is_spike, 0.1, 0.3) * (torch.rand(total, generator=g, dtype=torch.float64) * 2 - 1)
    return {"hidden": hidden, "obs_dim": D, "K": K, "gather": gather, "pols": pols, "spec": spec, "flat": torch.stack([p.flat for p in pols]).contiguous(),
            "obs": obs, "act": act.contiguous(), "old_logp": (logp64 + spread).float().contiguous(), "idx": idx, "spike_rows": spike_rows, "silent": silent,
            "mean64": mean64, "value64": value64, "logp64": logp64,
            "adv_spike": _signed((total,), 1.0, 2.0, g).float(), "ret_offset": _signed((total,), 1.0, 2.0, g), "teacher_offset": _signed((total, 7), 0.5, 1.0, g),
            "ret_any": (value64 + torch.randn(total, generator=g, dtype=torch.float64)).float()}


def _buf(c: dict, adv: torch.Tensor, ret: torch.Tensor) -> dict:
    return {"obs": c["obs"], "act": c["act"], "old_logp": c["old_logp"], "adv": adv.contiguous(), "ret": ret.contiguous()}


def policy_side(c: dict) -> dict:
    """run with vf_coef = 0: advantage 0 on the silent rows, random sign x [1, 2] on the spikes (and outside the selection)"""
    adv = c["adv_spike"].clone()
    adv[c["silent"]] = 0.0
    return _buf(c, adv, c["ret_any"])


def value_side(c: dict, own_value: torch.Tensor | None = None) -> dict:
    """run with vf_coef = 0.5 and advantage 0 everywhere: the return of a silent row is the value the handle itself computes for it
    (own_value [K][2065] by batch position; None: the fp64 value rounded to fp32, the CPU stand-in), that of a spike value + sign x [1, 2]"""
    ret = (c["value64"] + c["ret_offset"]).float()
    own = c["value64"].float() if own_value is None else None
    for r in range(c["K"]):
        rows = c["idx"][r]
        quiet = c["silent"][rows]
        ret[rows[quiet]] = own[rows[quiet]] if own_value is None else own_value[r].cpu()[quiet]
    return _buf(c, torch.zeros_like(c["adv_spike"]), ret)


def anchor_side(c: dict, own_mean: torch.Tensor | None = None) -> torch.Tensor:
    """teacher_actions [rows][7]: the handle's own deterministic mean on the silent rows (own_mean [K][2065][7]; None: fp64 mean rounded to
    fp32), mean + sign x [0.5, 1] per component on the spikes (and outside the selection)"""
    teacher = (c["mean64"] + c["teacher_offset"]).float()
    own = c["mean64"].float() if own_mean is None else None
    for r in range(c["K"]):
        rows = c["idx"][r]
        quiet = c["silent"][rows]
        teacher[rows[quiet]] = own[rows[quiet]] if own_mean is None else own_mean[r].cpu()[quiet]
    return teacher.contiguous()


# ------------------------------------------------------------------------------------------------ references
def loss_reference(c: dict, buf: dict, r: int, rows: torch.Tensor, vf_coef: float, count: int = NS) -> dict:
    """fp64 autograd of sum over `rows` of the PPO loss terms (raw advantages, no entropy term) / count, for replica r: what kp1_mlp_loss_grad
    computes with inv_count = 1 / count when every other row of its minibatch contributes nothing"""
    ref = S.reference(c["flat"][r], c["spec"], c["obs_dim"], buf, rows, clip_range=CLIP_RANGE, ent_coef=0.0, vf_coef=vf_coef, adv_mode="raw")
    ref["grad"] = ref["grad"] * (rows.numel() / count)
    return ref


def anchor_reference(c: dict, teacher: torch.Tensor, r: int, rows: torch.Tensor, n: int = N) -> dict:
    """fp64 autograd of LOSS_WEIGHT * sum_{i in rows, d < 7} (mean_d - teacher_d)^2 / (7 n): the kernel's mean over its n rows, of which
    only `rows` contribute"""
    f = c["flat"][r].double().clone().requires_grad_(True)
    mean, _ = P.mlp_forward(S.views_of(f, c["spec"]), c["obs"][rows, :c["obs_dim"]].double())
    loss = LOSS_WEIGHT * ((mean - teacher[rows].double()) ** 2).sum() / (7 * n)
    (grad,) = torch.autograd.grad(loss, f)
    return {"grad": grad, "loss": loss.item()}


def tolerances(ref_grad: torch.Tensor, spec) -> dict[str, float]:
    """the project's gradient tolerance for a comparison with torch autograd, per tensor: 2e-4 * max|ref| + 1e-7"""
    return {name: 2e-4 * (ref_grad[sl].abs().max().item() + 1e-12) + 1e-7 for name, sl in S.slices_of(spec).items()}


def grad_errors(grad: torch.Tensor, ref_grad: torch.Tensor, spec) -> dict[str, float]:
    """per tensor: max |grad - ref| / tolerance"""
    g, tol = grad.detach().cpu().double(), tolerances(ref_grad, spec)
    return {name: (g[sl] - ref_grad[sl]).abs().max().item() / tol[name] for name, sl in S.slices_of(spec).items()}


def active(side: str):
    """names of the tensors the run of this side reaches (the others must come out exactly 0)"""
    if side == "policy":
        return lambda name: name.startswith(POLICY)
    if side == "value":
        return lambda name: not name.startswith(POLICY)
    assert side == "anchor"
    return lambda name: name.startswith(ACTOR)


# ------------------------------------------------------------------------------------------------ approx_kl
def approx_kl_bound(flat: torch.Tensor, spec, obs_dim: int, obs: torch.Tensor, act: torch.Tensor, old_logp: torch.Tensor) -> dict:
    """approx_kl = mean((ratio - 1) - log ratio) of the given rows (CPU tensors) in fp64, and the bound of a fp32 evaluation of it:
        bound = 8 * max(e32, floor)          (adam_bounds' idiom)
    e32 = |the same expression with P.mlp_forward / P.gaussian_log_prob in float32 on the CPU - fp64|;
    floor = 2^-23 * max(1, max|logp|) * mean|log ratio|: log ratio = logp - old_logp inherits one fp32 spacing of the log-prob, at most
    2^-23 * max(1, max|logp|), and d kl / d log ratio = ratio - 1 ~ log ratio, so one spacing moves the mean by about spacing * mean|log ratio|."""
    flat, obs, act, old_logp = flat.detach().cpu(), obs.detach().cpu(), act.detach().cpu(), old_logp.detach().cpu()
    out = {}
    for dtype in (torch.float64, torch.float32):
        Pv = S.views_of(flat.to(dtype), spec)
        with torch.no_grad():
            mean, _ = P.mlp_forward(Pv, obs[:, :obs_dim].to(dtype).contiguous())
            logp = P.gaussian_log_prob(act.to(dtype), mean, Pv["log_std"])
            lr = logp - old_logp.to(dtype)
            out[dtype] = (((torch.exp(lr) - 1) - lr).mean().item(), logp.abs().max().item(), lr.abs().mean().item(), (0.5 * lr * lr).mean().item())
    kl64, max_logp, mean_lr, second_order = out[torch.float64]
    e32 = abs(out[torch.float32][0] - kl64)
    floor = 2.0 ** -23 * max(1.0, max_logp) * mean_lr
    return {"kl64": kl64, "e32": e32, "floor": floor, "bound": 8.0 * max(e32, floor), "second_order64": second_order}

