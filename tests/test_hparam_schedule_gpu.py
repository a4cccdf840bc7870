"""Hyper-parameters read from device memory, and the learning-rate / clip-range schedules on top of them.

Every comparison here is bit for bit against a twin -- a handle or a trainer -- that receives the same values as scalar arguments.  The
scalars handed to a handle whose line is on are deliberately other (finite) values: were any of them read, the twins would differ."""
from __future__ import annotations

import ctypes as C
import zipfile

import pytest
import torch

import mlp_handle_state as S
from rl_brain_trainer_amd import native

pytestmark = pytest.mark.gpu
DEV = S.DEV
FIELDS = ("learning_rate", "adam_eps", "max_grad_norm", "clip_range", "ent_coef", "vf_coef")
H1 = dict(learning_rate=3e-3, adam_eps=1e-5, max_grad_norm=0.5, clip_range=0.2, ent_coef=1e-2, vf_coef=0.5)
H2 = dict(learning_rate=1e-3, adam_eps=1e-6, max_grad_norm=0.3, clip_range=0.1, ent_coef=3e-2, vf_coef=0.7)
H3 = dict(learning_rate=2e-2, adam_eps=1e-4, max_grad_norm=1.5, clip_range=0.3, ent_coef=0.0, vf_coef=0.25)
WRONG = dict(learning_rate=7e-2, adam_eps=1e-3, max_grad_norm=5.0, clip_range=0.45, ent_coef=0.2, vf_coef=0.1)     # what a line must hide
KP1_ERR_INVALID, KP1_ERR_UNSUPPORTED = -1, -4


def _same(a, b) -> bool:
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


class _World:
    """one handle kind: start parameters, sample buffers and two minibatches of n rows"""

    def __init__(self, hidden: int, obs_dim: int, path: str, n: int, *, tile: bool = False):
        self.kind, self.n, self.tile = (hidden, obs_dim, path), n, tile
        self.pol = S.policy(hidden, obs_dim)
        self.flat0 = self.pol.flat.to(DEV)
        self.buf = S.dev(S.sample_buffers(self.pol.flat, self.pol.spec, obs_dim, seed=1))
        self.sels = [S.selection(S.TOTAL, n, 10 + i).to(DEV) for i in range(3)]

    def handle(self, replicas: int = 1):
        k = S.handle(self.kind, max_batch=max(128, self.n), replicas=replicas)
        if self.tile:
            k.set_train_tile(True)
        return k


class _Run:
    def __init__(self, w: _World, k, replicas: int = 1):
        self.w, self.k, self.K = w, k, replicas
        self.p = w.flat0.repeat(replicas).contiguous()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.grad = torch.full_like(self.p, float("nan"))
        self.stats = torch.zeros(4 * replicas, device=DEV)
        k.pack(self.p)

    def pair(self, idx, h: dict, stats=None) -> None:
        """loss_grad + adam_step with h's values as the scalar arguments"""
        S.loss_grad(self.k, self.w.buf, idx, self.w.n, self.grad, self.stats if stats is None else stats, clip_range=h["clip_range"],
                    ent_coef=h["ent_coef"], vf_coef=h["vf_coef"])
        self.k.adam_step(self.p, self.grad, self.m, self.v, lr=h["learning_rate"], eps=h["adam_eps"], max_grad_norm=h["max_grad_norm"], step=0,
                         fused_norm=True)

    def forward(self):
        obs = self.w.buf["obs"][:64].repeat(self.K, 1).contiguous()
        mean, value = torch.empty((64 * self.K, 7), device=DEV), torch.empty(64 * self.K, device=DEV)
        self.k.forward(obs, mean=mean, value=value)
        return [mean, value]

    def all(self):
        """gradient, statistics, parameters, both moments, and a forward on the repacked weights"""
        return [t.clone() for t in (self.grad, self.stats, self.p, self.m, self.v)] + self.forward()


# ================================================================================================ kernel level, K = 1
SHAPES = {
    "layer-64": (64, 56, "layer", 64, False), "layer-128": (128, 56, "layer", 64, False),
    "train-tile-64": (64, 56, "layer", 64, True), "train-tile-128": (128, 56, "layer", 64, True),
    "layer-128-obs80": (128, 80, "layer", 64, False), "train-tile-128-obs80": (128, 80, "layer", 64, True),
    "tile-2x256": (256, 56, "fused", 256, False), "tile-2x256-obs80": (256, 80, "fused", 256, False),
    "layer-256": (256, 56, "layer", 64, False),
    # 33 rows: one full 32-row tile and one that holds a single row
    "tile-2x256-33rows": (256, 56, "fused", 33, False), "train-tile-64-33rows": (64, 56, "layer", 33, True), "layer-256-33rows": (256, 56, "layer", 33, False),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_line_equals_scalars(shape):
    """hparams_store([h]), a pair called with other scalars, hparams_store([h2]), a second pair -- against a handle without a line that gets
    h's, then h2's scalars"""
    hidden, obs_dim, path, n, tile = SHAPES[shape]
    w = _World(hidden, obs_dim, path, n, tile=tile)
    kt, kl = w.handle(), w.handle()
    twin, line = _Run(w, kt), _Run(w, kl)
    assert not kl.hparam_line
    kl.hparams_store([H1])
    assert kl.hparam_line
    twin.pair(w.sels[0], H1)
    line.pair(w.sels[0], WRONG)
    first = (twin.all(), line.all())
    assert _same(*first), f"{shape}: the first pair differs"
    kl.hparams_store([H2])
    twin.pair(w.sels[1], H2)
    line.pair(w.sels[1], WRONG)
    assert _same(twin.all(), line.all()), f"{shape}: the second pair differs"
    assert not _same(first[0][2:3], [twin.p])      # (the second pair moved the parameters)
    # and the values matter: the twin called with the scalars the line hid ends elsewhere
    kw = w.handle()
    wrong = _Run(w, kw)
    wrong.pair(w.sels[0], WRONG)
    assert not _same(wrong.all()[2:3], first[0][2:3])
    for k in (kt, kl, kw):
        k.close()


# one field off at a time.  Two of WRONG's values are replaced by ones that bite on any minibatch: a clip range of 0.02 cuts every row whose
# ratio left [0.98, 1.02] on its advantage's side (0.45 would need one beyond 1.2), and a norm bound of 0.01 scales every gradient longer
# than that (5.0 scales none shorter than 5)
ONE_OFF = dict(WRONG, clip_range=0.02, max_grad_norm=0.01)


@pytest.mark.parametrize("shape", ["layer-64", "train-tile-64", "tile-2x256", "tile-2x256-obs80", "layer-256"])
def test_each_field_is_read_from_the_line(shape):
    """one variant per field: the line holds h, the scalars equal h in every field but one.  The handle with the line must end where
    h's scalar twin ends, and a scalar handle given those same mixed scalars must end elsewhere -- so a kernel that took that one field
    from its arguments would be caught by the first comparison"""
    hidden, obs_dim, path, n, tile = SHAPES[shape]
    w = _World(hidden, obs_dim, path, n, tile=tile)
    kt = w.handle()
    twin = _Run(w, kt)
    twin.pair(w.sels[0], H1)
    ref = twin.all()
    kt.close()
    for f in FIELDS:
        mixed = dict(H1, **{f: ONE_OFF[f]})
        kl, ks = w.handle(), w.handle()
        line, scalar = _Run(w, kl), _Run(w, ks)
        kl.hparams_store([H1])
        line.pair(w.sels[0], mixed)
        scalar.pair(w.sels[0], mixed)
        assert _same(line.all(), ref), f"{shape}: {f} was not read from the line"
        assert not _same(scalar.all()[2:3], ref[2:3]), f"{shape}: {f} = {ONE_OFF[f]} moves no parameter here, the variant shows nothing"
        kl.close()
        ks.close()


def test_population_lines():
    """K = 3 with three distinct lines: hparams_store against set_replica_hparams on a twin, and replica 1 against a K = 1 scalar handle"""
    K, rows = 3, [H1, H2, H3]
    w = _World(64, 56, "layer", 64)
    ka, kb, k1 = w.handle(K), w.handle(K), w.handle()
    a, b, one = _Run(w, ka, K), _Run(w, kb, K), _Run(w, k1)
    ka.hparams_store(rows)
    kb.set_replica_hparams(rows)
    sels = [[S.selection(S.TOTAL, w.n, 100 * r + i).to(DEV) for i in range(2)] for r in range(K)]
    for i in range(2):
        idx = torch.stack([sels[r][i] for r in range(K)]).contiguous()
        a.pair(idx, WRONG)
        b.pair(idx, WRONG)
        one.pair(sels[1][i], rows[1])
        if i == 0:      # a new table between the pairs, through either entry point
            rows = [H2, H3, H1]
            ka.hparams_store(rows)
            kb.set_replica_hparams(rows)
    assert _same(a.all(), b.all())
    P = one.p.numel()
    rep1 = [a.grad[P:2 * P], a.stats[4:8], a.p[P:2 * P], a.m[P:2 * P], a.v[P:2 * P]]
    assert _same(rep1, [one.grad, one.stats, one.p, one.m, one.v])
    for k in (ka, kb, k1):
        k.close()


@pytest.mark.parametrize("form", ["layer-64", "tile-2x256"])
def test_captured_pair_reads_the_line_at_replay(form):
    """[loss_grad, adam_step] captured once with the line on; replay, hparams_store([h2]), replay -- the eager twin with h, then h2"""
    hidden, obs_dim, path, n, tile = SHAPES[form]
    w = _World(hidden, obs_dim, path, n)
    kt, kl = w.handle(), w.handle()
    twin, line = _Run(w, kt), _Run(w, kl)
    kl.hparams_store([H1])
    twin.pair(w.sels[0], H1)
    line.pair(w.sels[0], WRONG)          # once eagerly: the kernels are loaded and their attributes set before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        line.pair(w.sels[1], WRONG)
    g.replay()
    twin.pair(w.sels[1], H1)
    assert _same(twin.all(), line.all())
    kl.hparams_store([H2])               # eagerly: the graph holds the line's address
    g.replay()
    twin.pair(w.sels[1], H2)
    assert _same(twin.all(), line.all())
    kt.close()
    kl.close()


def _threshold(trace: list[float], pos: int) -> float:
    """1.5 * target for a stop at ``pos``, as tests/test_kl_gate_gpu.py derives it: midway between the largest value before it and the value
    at it, the first crossing, and no trace value within 1e-3 relative of it"""
    before = max(trace[:pos], default=0.0)
    assert trace[pos] > before > -1e-6, f"the twin's KL trace does not reach a new maximum at {pos}: {trace}"
    thr = 0.5 * (max(before, 0.0) + trace[pos])
    assert [i for i, v in enumerate(trace) if v > thr][0] == pos
    assert all(abs(v - thr) > 1e-3 * thr for v in trace), (trace, thr)
    return thr


def test_kl_gate_on_a_line():
    """a gated K = 1 handle with a line against a gated handle driven with scalars: the gated finalize and Adam forms read the line too"""
    w = _World(64, 56, "layer", 64)
    h = dict(H1, learning_rate=3e-2)          # large on purpose: the KL trace has to rise
    ku = w.handle()
    un, trace = _Run(w, ku), []
    for idx in w.sels:
        st = torch.zeros(4, device=DEV)
        un.pair(idx, h, st)
        trace.append(float(st[3]))            # 0 + kl exactly: the float the device compares
    ku.close()
    thr = _threshold(trace, 1)
    kt, kl = w.handle(), w.handle()
    kt.set_kl_gate([thr / 1.5])
    kl.set_kl_gate([thr / 1.5])
    kl.hparams_store([h])
    twin, line = _Run(w, kt), _Run(w, kl)
    for idx in w.sels:
        twin.pair(idx, h)
        line.pair(idx, WRONG)
    assert _same(twin.all(), line.all())
    (rt,), st_t = kt.kl_gate_read()
    (rl,), st_l = kl.kl_gate_read()
    assert rt == rl and st_t == st_l == [1] and (rl["stopped"], rl["n_counted"], rl["n_seen"], rl["stop_index"]) == (1, 2, 3, 1)
    assert rl["stop_kl"] == trace[1]
    kt.close()
    kl.close()


def test_clearing_returns_to_the_scalars():
    w = _World(64, 56, "layer", 64)
    kt, kl = w.handle(), w.handle()
    twin, line = _Run(w, kt), _Run(w, kl)
    kl.hparams_store([WRONG])
    kl.set_replica_hparams(None)
    assert not kl.hparam_line
    twin.pair(w.sels[0], H1)
    line.pair(w.sels[0], H1)
    assert _same(twin.all(), line.all())
    with pytest.raises(native.Kp1Error, match="K = 1"):       # the older entry point keeps its refusal
        kl.set_replica_hparams([H1])
    kt.close()
    kl.close()


def _table(rows):
    return (C.c_float * (6 * len(rows)))(*[float(r[f]) for r in rows for f in FIELDS])


def test_refusals_leave_the_handle_untouched():
    w = _World(64, 56, "layer", 64)
    k = w.handle()
    L, h, st = k.L, k._h, k._stream()
    err = lambda: L.kp1_last_error().decode()      # noqa: E731
    one = C.cast(_table([H1]), C.c_void_p)
    assert L.kp1_mlp_hparams_store(None, one, 1, st) == KP1_ERR_INVALID and "NULL" in err()
    assert L.kp1_mlp_hparams_store(h, None, 1, st) == KP1_ERR_INVALID and "NULL" in err()
    for n in (0, 2, -1):
        assert L.kp1_mlp_hparams_store(h, C.cast(_table([H1, H2]), C.c_void_p), n, st) == KP1_ERR_INVALID and "n = K" in err()
    for f in FIELDS:
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert L.kp1_mlp_hparams_store(h, C.cast(_table([dict(H1, **{f: bad})]), C.c_void_p), 1, st) == KP1_ERR_INVALID and "finite" in err(), f
    with pytest.raises(ValueError, match="n = K"):
        k.hparams_store([H1, H2])
    assert not k.hparam_line
    k3 = w.handle(3)
    assert L.kp1_mlp_hparams_store(k3._h, C.cast(_table([H1]), C.c_void_p), 1, st) == KP1_ERR_INVALID and "n = K" in err()
    assert L.kp1_mlp_hparams_store(k3._h, C.cast(_table([H1, H2, dict(H3, clip_range=float("nan"))]), C.c_void_p), 3, st) == KP1_ERR_INVALID
    k3.close()
    # still a handle on its scalars: one pair equals a fresh handle's
    run = _Run(w, k)
    run.pair(w.sels[0], H1)
    kf = w.handle()
    fresh = _Run(w, kf)
    fresh.pair(w.sels[0], H1)
    assert _same(run.all(), fresh.all())
    # the anchor entry points on a K = 1 line: their K = 1 forms read scalars
    k.hparams_store([H1])
    before = run.all()
    loss, teacher = torch.zeros(1, device=DEV), torch.zeros((S.TOTAL, 7), device=DEV)
    agrad = torch.zeros_like(run.grad)
    with pytest.raises(native.Kp1Error, match=f"kp1 error {KP1_ERR_UNSUPPORTED}: .*hyper-parameter line"):
        k.anchor_loss_grad(w.buf["obs"], w.sels[0], w.n, teacher, loss_weight=1.0, grad_out=agrad, loss_out=loss)
    with pytest.raises(native.Kp1Error, match=f"kp1 error {KP1_ERR_UNSUPPORTED}: .*hyper-parameter line"):
        k.anchor_adam_step(run.p, agrad, run.m, run.v, lr=1e-3, eps=1e-5, max_grad_norm=0.5, step=0)
    assert _same(run.all(), before) and float(agrad.abs().max()) == 0.0 and float(loss) == 0.0
    k.set_replica_hparams(None)          # ... and are back once the line is cleared
    k.anchor_loss_grad(w.buf["obs"], w.sels[0], w.n, teacher, loss_weight=1.0, grad_out=agrad, loss_out=loss)
    assert float(agrad.abs().max()) > 0.0
    k.close()
    kf.close()


def test_bf16x3_has_no_line_form():
    w = _World(256, 56, "fused", 64)
    k = w.handle()
    k.set_bf16x3_wgrad(True)
    with pytest.raises(native.Kp1Error, match=f"kp1 error {KP1_ERR_UNSUPPORTED}: .*bf16x3.*line"):
        k.hparams_store([H1])
    assert not k.hparam_line
    k.set_bf16x3_wgrad(False)
    k.hparams_store([H1])
    with pytest.raises(native.Kp1Error, match=f"kp1 error {KP1_ERR_UNSUPPORTED}: .*bf16x3.*line"):
        k.set_bf16x3_wgrad(True)
    # untouched by either refusal: the exact path with the line equals a scalar twin
    kt = w.handle()
    twin, line = _Run(w, kt), _Run(w, k)
    twin.pair(w.sels[0], H1)
    line.pair(w.sels[0], WRONG)
    assert _same(twin.all(), line.all())
    k.close()
    kt.close()


# ================================================================================================ trainer level
N_ENVS = 16
LR_SCHED, CLIP_SCHED = {"end": 0.0, "end_fraction": 1.0}, {"end": 0.05, "end_fraction": 0.5}


def _linear(start: float, end: float, end_fraction: float, p: float) -> float:
    """stable_baselines3.common.utils.LinearSchedule.__call__, restated"""
    if (1 - p) > end_fraction:
        return end
    return start + (1 - p) * (end - start) / end_fraction


@pytest.fixture(scope="module")
def env_cfg():
    from rl_brain_trainer_amd import config as kcfg

    return kcfg.to_env_config(kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"))


def _pcfg(hidden: int = 64, n_steps: int = 64, seed: int = 7, scheduled: bool = True, **kw):
    from rl_brain_trainer_amd.ppo import PPOConfig

    if scheduled:
        kw = dict(dict(learning_rate_schedule=dict(LR_SCHED), clip_range_schedule=dict(CLIP_SCHED)), **kw)
    return PPOConfig(**dict(dict(n_steps=n_steps, batch_size=256, n_epochs=2, hidden=hidden, learning_rate=3e-4, clip_range=0.2, ent_coef=1e-3, seed=seed), **kw))


def _trainer(env_cfg, cfg, **kw):
    from rl_brain_trainer_amd.ppo import PPO
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    return PPO(ArmKinematicVecEnv(env_cfg, N_ENVS, seed=cfg.seed), cfg, **kw)


def _count_epoch_captures(ppo) -> list[str]:
    calls, orig = [], ppo._capture

    def counted(body, on_begin=None):
        calls.append(getattr(body, "__name__", "rollout"))
        return orig(body, on_begin=on_begin)

    ppo._capture = counted
    return calls


def _snapshot(ppo) -> dict:
    return {"state": [t.clone() for t in (ppo.policy.flat, ppo.adam_m, ppo.adam_v)], "adam_t": ppo.adam_t, "stats": dict(ppo.last_stats)}


def _scheduled_against_twin(env_cfg, hidden: int, n_steps: int, iterations: int, use_graphs: bool):
    from rl_brain_trainer_amd.ppo import run_training

    per_it = N_ENVS * n_steps
    total = iterations * per_it
    sched = _trainer(env_cfg, _pcfg(hidden, n_steps), use_graphs=use_graphs)
    caps = _count_epoch_captures(sched)
    got, used = [], []

    def after_update(tr, steps):
        got.append(_snapshot(tr))
        used.append((tr.progress_remaining, tr.current_hparams()))

    run_training(sched, total, after_update=after_update)
    assert sched._mlp.hparam_line and len(got) == iterations
    twin = _trainer(env_cfg, _pcfg(hidden, n_steps, scheduled=False), use_graphs=use_graphs)
    twin_caps = _count_epoch_captures(twin)
    branches = []
    for it in range(iterations):
        twin.collect_rollouts()
        p = 1.0 - float(twin.num_timesteps) / float(total)
        twin.cfg.learning_rate = _linear(3e-4, LR_SCHED["end"], LR_SCHED["end_fraction"], p)
        twin.cfg.clip_range = _linear(0.2, CLIP_SCHED["end"], CLIP_SCHED["end_fraction"], p)
        branches.append("end" if (1 - p) > CLIP_SCHED["end_fraction"] else "interpolated")
        assert used[it] == (p, {"learning_rate": twin.cfg.learning_rate, "clip_range": twin.cfg.clip_range}), it
        twin.train()
        want = _snapshot(twin)
        assert _same(got[it]["state"], want["state"]), f"iteration {it}: parameters or moments differ"
        assert got[it]["adam_t"] == want["adam_t"] and got[it]["stats"] == want["stats"], it
        assert not twin._mlp.hparam_line
    out = {"caps": caps.count("_epoch_body"), "twin_caps": twin_caps.count("_epoch_body"), "branches": branches}
    sched.env.close()
    twin.env.close()
    return out


@pytest.mark.parametrize("use_graphs", [True, False], ids=["graphs", "eager"])
def test_scheduled_trainer_hidden_64(env_cfg, use_graphs):
    """three iterations of run_training under both schedules against an unscheduled trainer whose cfg the test sets before each train()
    from the restated formula; the scheduled trainer captures its epoch graph once, the twin once per new value"""
    out = _scheduled_against_twin(env_cfg, 64, 64, 3, use_graphs)
    assert out["branches"] == ["interpolated", "end", "end"]
    assert (out["caps"], out["twin_caps"]) == ((1, 3) if use_graphs else (0, 0))


def test_scheduled_trainer_hidden_256(env_cfg):
    """the 2x256 tile path: mlp_tile_line_kernel inside the captured epoch, two iterations"""
    out = _scheduled_against_twin(env_cfg, 256, 16, 2, True)
    assert out["branches"] == ["interpolated", "end"] and (out["caps"], out["twin_caps"]) == (1, 2)


def test_population_trainer_against_single_trainers(env_cfg):
    """ApproachPopulationPPO, K = 2, two start learning rates and a shared schedule: each replica equals the single scheduled trainer of its
    seed and start"""
    from rl_brain_trainer_amd.population import ApproachPopulationPPO
    from rl_brain_trainer_amd.ppo import run_training
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    seeds, lrs, total = [7, 8], [3e-4, 1e-3], 2 * N_ENVS * 64
    penv = ArmKinematicPopulationVecEnv(env_cfg, seeds, N_ENVS)
    pop = ApproachPopulationPPO(seeds, _pcfg(), penv, overrides=[{"learning_rate": lr} for lr in lrs])
    run_training(pop, total)
    p = pop.progress_remaining
    assert p == 0.0
    rows = pop._stats_rows()
    for k, (s, lr) in enumerate(zip(seeds, lrs)):
        assert pop.current_hparams(k) == {"learning_rate": _linear(lr, 0.0, 1.0, p), "clip_range": _linear(0.2, 0.05, 0.5, p)}
        single = _trainer(env_cfg, _pcfg(seed=s, learning_rate=lr))
        run_training(single, total)
        assert _same([pop.flat[k], pop.adam_m[k], pop.adam_v[k]], [single.policy.flat, single.adam_m, single.adam_v]), k
        one = single.last_stats
        assert all(rows[k][q] == one[q] for q in ("policy_loss", "value_loss", "entropy", "approx_kl", "n_updates")), (k, rows[k], one)
        assert pop.replica(k).current_hparams() == single.current_hparams()
        single.env.close()
    pop.close()


def test_resume_clock_monitor_and_checkpoint(env_cfg, tmp_path):
    """a trainer whose clock starts at c0 > 0 uses 1 - n / (c0 + R); monitor_rows() and the checkpoint carry the current values"""
    from rl_brain_trainer_amd import checkpoint
    from rl_brain_trainer_amd import sb3_pickle as sbp
    from rl_brain_trainer_amd.ppo import run_training

    c0, R, per_it = 5000, 2048, N_ENVS * 64
    ppo = _trainer(env_cfg, _pcfg(), monitor=True)
    ppo.num_timesteps = c0
    seen = []
    run_training(ppo, R, after_update=lambda tr, steps: seen.append((tr.progress_remaining, tr.current_hparams())))
    ps = [1.0 - float(c0 + (i + 1) * per_it) / float(c0 + R) for i in range(2)]
    assert [s[0] for s in seen] == ps and ps[1] == 0.0 and 0.0 < ps[0] < 1.0
    assert [s[1] for s in seen] == [{"learning_rate": _linear(3e-4, 0.0, 1.0, p), "clip_range": _linear(0.2, 0.05, 0.5, p)} for p in ps]
    row = ppo.monitor_rows()[0]
    assert row["train/learning_rate"] == seen[-1][1]["learning_rate"] == 0.0 and row["train/clip_range"] == seen[-1][1]["clip_range"] == 0.05
    # one more update at a progress the caller sets itself
    ppo.collect_rollouts()
    ppo.progress_remaining = 0.75
    ppo.train()
    now = {"learning_rate": _linear(3e-4, 0.0, 1.0, 0.75), "clip_range": _linear(0.2, 0.05, 0.5, 0.75)}
    row = ppo.monitor_rows()[0]
    assert (row["train/learning_rate"], row["train/clip_range"]) == (now["learning_rate"], now["clip_range"])
    path = checkpoint.save(tmp_path / "scheduled", ppo, env_cfg)
    data = checkpoint.load_data(path)
    assert data["learning_rate"] == 3e-4 and data["_current_progress_remaining"] == 0.75
    for key, start, s in (("lr_schedule", 3e-4, LR_SCHED), ("clip_range", 0.2, CLIP_SCHED)):
        e = data[key]
        assert (e["value"], e["end"], e["end_fraction"]) == (start, s["end"], s["end_fraction"])
        assert e[":serialized:"] == sbp.serialized(sbp.linear_schedule(start, s["end"], s["end_fraction"]))
        assert sbp.describe(e[":serialized:"])[1] == ("stable_baselines3.common.utils", "LinearSchedule")
    assert checkpoint.load_optimizer_state_dict(path)["param_groups"][0]["lr"] == now["learning_rate"]
    ppo.env.close()
    ppo.monitor.close()


def test_unscheduled_trainer_is_the_parent(env_cfg, tmp_path):
    """both fields None: no hparams_store call, no line, the key of a trainer built without the fields, and the same archive bytes"""
    from rl_brain_trainer_amd import checkpoint
    from rl_brain_trainer_amd.ppo import PPOConfig

    bare = PPOConfig(n_steps=64, batch_size=256, n_epochs=2, hidden=64, learning_rate=3e-4, clip_range=0.2, ent_coef=1e-3, seed=7)
    members, keys = [], []
    for name, cfg in (("none", _pcfg(scheduled=False, learning_rate_schedule=None, clip_range_schedule=None)), ("bare", bare)):
        ppo = _trainer(env_cfg, cfg)
        stores, orig = [], ppo._mlp.hparams_store
        ppo._mlp.hparams_store = lambda rows: (stores.append(rows), orig(rows))
        ppo.collect_rollouts()
        ppo.progress_remaining = 0.5
        ppo.train()
        assert not stores and not ppo._mlp.hparam_line and ppo.hparam_schedules is None
        assert ppo.current_hparams() == {"learning_rate": 3e-4, "clip_range": 0.2}
        keys.append(ppo._epoch_key())
        with zipfile.ZipFile(checkpoint.save(tmp_path / name, ppo, env_cfg)) as z:
            members.append({n: z.read(n) for n in z.namelist()})
        ppo.env.close()
    assert keys[0] == keys[1] and len(keys[0]) == 11 and not any(isinstance(e, tuple) for e in keys[0])
    assert members[0] == members[1]
    data = members[0]["data"].decode()
    assert '"_current_progress_remaining": 1.0' in data and '"end_fraction"' not in data
