"""PPO's target_kl as a device decision: the gated forms of the finalize and Adam launches, the handle's entry points and
the trainers on top of them.  Everything here is bit equality against an ungated run of the same calls, cut where SB3's loop would break.

The stop threshold of every case is derived from an ungated twin, never written down: the twin is driven minibatch by minibatch with a freshly
zeroed stats_out, so its stats[3] is 0 + kl exactly -- the float the device compares -- and 1.5 * target is put midway between the largest
trace value before the wanted position and the value at it (``_threshold``, which also asserts that the position is the first crossing and
that no trace value lies within 1e-3 relative of the threshold).  The learning rates are large on purpose: the KL trace has to rise."""
from __future__ import annotations

import math

import pytest
import torch

import mlp_handle_state as S
from rl_brain_trainer_amd import native

pytestmark = pytest.mark.gpu
DEV = S.DEV
ADAM = dict(lr=3e-2, eps=1e-5, max_grad_norm=0.5)


def _threshold(trace: list[float], pos: int) -> float:
    """1.5 * target for a stop at ``pos``: midway between the largest value before it and the value at it"""
    before = max(trace[:pos], default=0.0)
    assert trace[pos] > before > -1e-6, f"the twin's KL trace does not reach a new maximum at {pos}: {trace}"
    thr = 0.5 * (max(before, 0.0) + trace[pos])
    assert [i for i, v in enumerate(trace) if v > thr][0] == pos
    assert all(abs(v - thr) > 1e-3 * thr for v in trace), (trace, thr)
    return thr


def _first_new_maximum(trace: list[float], candidates) -> int:
    found = [i for i in candidates if trace[i] > max(trace[:i], default=0.0)]
    assert found, f"no new maximum of the KL trace at any of {list(candidates)}: {trace}"
    return found[0]


# ================================================================================================ kernel level
class _World:
    """one handle kind: start parameters, sample buffers and the minibatches (row selections) of a case"""

    def __init__(self, hidden: int, n: int, *, tile: bool = False, pairs: int = 3):
        self.hidden, self.n, self.tile = hidden, n, tile
        self.kind = (hidden, 56, "fused" if hidden == 256 else "layer")
        self.pol = S.policy(hidden, 56)
        self.flat0 = self.pol.flat.to(DEV)
        self.buf = S.dev(S.sample_buffers(self.pol.flat, self.pol.spec, 56, seed=1))
        self.sels = [S.selection(S.TOTAL, n, 10 + i).to(DEV) for i in range(pairs)]

    def handle(self, targets="ungated", replicas: int = 1):
        k = S.handle(self.kind, max_batch=max(128, self.n), replicas=replicas)
        if self.tile:
            k.set_train_tile(True)
        if targets != "ungated":
            k.set_kl_gate(targets)
        return k


class _Run:
    """parameters, Adam moments, gradient and accumulated statistics of one handle"""

    def __init__(self, w: _World, k, replicas: int = 1):
        self.w, self.k, self.K = w, k, replicas
        self.p = w.flat0.repeat(replicas).contiguous()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.grad = torch.full_like(self.p, float("nan"))
        self.stats = torch.zeros(4 * replicas, device=DEV)
        k.pack(self.p)

    def loss_grad(self, idx, stats=None):
        S.loss_grad(self.k, self.w.buf, idx, self.w.n, self.grad, self.stats if stats is None else stats)

    def adam(self):
        self.k.adam_step(self.p, self.grad, self.m, self.v, step=0, fused_norm=True, **ADAM)

    def pair(self, idx, stats=None):
        self.loss_grad(idx, stats)
        self.adam()

    def forward(self):
        obs = self.w.buf["obs"][:64].repeat(self.K, 1).contiguous()
        mean, value = torch.empty((64 * self.K, 7), device=DEV), torch.empty(64 * self.K, device=DEV)
        self.k.forward(obs, mean=mean, value=value)
        return mean, value

    def state(self):
        return [t.clone() for t in (self.p, self.m, self.v)]


def _same(a, b) -> bool:
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _twin_trace(w: _World, sels=None) -> list[float]:
    """the ungated twin: per pair a freshly zeroed stats_out, whose [3] is then 0 + kl exactly"""
    k = w.handle()
    run, trace = _Run(w, k), []
    for idx in (w.sels if sels is None else sels):
        st = torch.zeros(4, device=DEV)
        run.pair(idx, st)
        trace.append(float(st[3]))
    k.close()
    return trace


def _stop_at_the_second_of_three(w: _World) -> None:
    trace = _twin_trace(w)
    thr = _threshold(trace, 1)
    # ungated: the first pair, then only the loss statistics of the second minibatch (SB3 logs them before it tests the KL)
    ku = w.handle()
    ref = _Run(w, ku)
    ref.pair(w.sels[0])
    after_first = ref.state()
    ref.loss_grad(w.sels[1])
    kg = w.handle([thr / 1.5])
    run = _Run(w, kg)
    for idx in w.sels:
        run.pair(idx)
    assert _same(run.state(), after_first), "a stopped replica's parameters or moments moved"
    assert _same(run.forward(), ref.forward()), "the packed weights of a stopped replica moved"
    assert _same([run.stats], [ref.stats]), (run.stats.tolist(), ref.stats.tolist())
    rec, steps = kg.kl_gate_read()
    assert steps == [1]
    r = rec[0]
    assert (r["stopped"], r["n_counted"], r["n_seen"], r["stop_index"]) == (1, 2, 3, 1), r
    assert r["stop_kl"] == trace[1] and r["threshold"] == 1.5 * (thr / 1.5)
    kg.kl_gate_arm()
    rec, steps = kg.kl_gate_read()
    r = rec[0]
    assert (r["stopped"], r["n_counted"], r["n_seen"], r["stop_index"], r["stop_kl"]) == (0, 0, 0, 0, 0.0) and steps == [1]
    assert r["threshold"] == 1.5 * (thr / 1.5)
    # armed again, the gate decides anew.  The ungated handle takes the next pair from the same state at count 2 and says what its KL is
    # (a minibatch seen before, at moved parameters: it may well lie above the threshold again)
    ku.set_step_count(1)
    st = torch.zeros(4, device=DEV)
    ref.pair(w.sels[0], st)
    kl_next = float(st[3])
    assert abs(kl_next - thr) > 1e-3 * thr
    run.stats.zero_()
    run.pair(w.sels[0])
    if kl_next > thr:      # stopped again, at the first minibatch since the arm: nothing moved
        rec, steps = kg.kl_gate_read()
        assert steps == [1] and (rec[0]["stopped"], rec[0]["n_counted"], rec[0]["n_seen"], rec[0]["stop_index"]) == (1, 1, 1, 0)
        assert rec[0]["stop_kl"] == kl_next and _same(run.state(), after_first)
        kg.set_kl_gate([4.0 * kl_next / 1.5])      # a target above it (setting one arms the records and keeps the step counts)
        run.stats.zero_()
        run.pair(w.sels[0])
    assert _same(run.state() + [run.stats], ref.state() + [st]) and not _same(run.state(), after_first)
    rec, steps = kg.kl_gate_read()
    assert steps == [2] and (rec[0]["stopped"], rec[0]["n_counted"], rec[0]["n_seen"]) == (0, 1, 1)
    ku.close()
    kg.close()


FORMS = {"layer-64": (64, 64, False), "train-tile-64": (64, 64, True), "train-tile-128": (128, 64, True), "tile-2x256": (256, 256, False)}


@pytest.mark.parametrize("form", list(FORMS))
def test_stop_at_the_second_of_three_pairs(form):
    """three loss_grad + adam_step pairs with a threshold that trips at the second: the handle is left as after the first pair, with the
    statistics of two minibatches -- on the layer-wise launches, on the training tile (hidden 64 and 128) and on the 2x256 tile path,
    which all end in the one finalize launch"""
    hidden, n, tile = FORMS[form]
    w = _World(hidden, n, tile=tile)
    if tile:
        k = w.handle()
        assert k.train_tile
        k.close()
    _stop_at_the_second_of_three(w)


def test_a_gate_without_a_target_changes_nothing():
    """threshold +inf (no target), NaN, 0 and a negative target: bit-equal to an ungated handle over the same calls"""
    w = _World(64, 64)
    ku = w.handle()
    ref = _Run(w, ku)
    for idx in w.sels:
        ref.pair(idx)
    for target in (None, float("nan"), 0.0, -0.01, float("inf")):
        kg = w.handle([target])
        run = _Run(w, kg)
        for idx in w.sels:
            run.pair(idx)
        assert _same(run.state() + [run.stats, run.grad], ref.state() + [ref.stats, ref.grad]), target
        rec, steps = kg.kl_gate_read()
        assert steps == [3] and (rec[0]["stopped"], rec[0]["n_counted"], rec[0]["n_seen"]) == (0, 3, 3) and math.isinf(rec[0]["threshold"])
        kg.set_kl_gate(None)      # K = 1: one count, the gate clears
        run.pair(w.sels[0])
        kg.close()
    ku.close()


def test_refusals_leave_the_handle_untouched():
    w = _World(64, 64)
    k = w.handle()
    L, h, st = k.L, k._h, k._stream()
    two = (native.C.c_double * 2)(0.01, 0.02)
    assert L.kp1_mlp_set_kl_gate(None, two, 1, st) != 0 and L.kp1_mlp_kl_gate_arm(None, st) != 0 and L.kp1_mlp_kl_gate_read(None, None, None, st) != 0
    assert L.kp1_mlp_set_kl_gate(h, None, 1, st) != 0                                  # NULL targets
    with pytest.raises(ValueError, match="n = K"):
        k.set_kl_gate([0.01, 0.02])                                                    # n != K
    with pytest.raises(ValueError, match="no KL gate"):
        k.kl_gate_arm()
    with pytest.raises(ValueError, match="no KL gate"):
        k.kl_gate_read()
    k.set_actor_extra_steps(2)
    with pytest.raises(native.Kp1Error, match="extra steps"):
        k.set_kl_gate([0.01])
    k.set_actor_extra_steps(0)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g.capture_begin()
        try:
            with pytest.raises(ValueError, match="captured"):
                k.set_kl_gate([0.01])
        finally:
            g.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    assert not k.kl_gate
    # still an ungated handle at count 0: one pair equals a fresh handle's
    run = _Run(w, k)
    run.pair(w.sels[0])
    fresh_k = w.handle()
    fresh = _Run(w, fresh_k)
    fresh.pair(w.sels[0])
    assert _same(run.state() + [run.stats], fresh.state() + [fresh.stats])
    # a gated handle: the anchor step and a non-zero actor extra count are not covered
    k.set_kl_gate([0.01])
    before = run.state()
    loss = torch.zeros(1, device=DEV)
    teacher = torch.zeros((S.TOTAL, 7), device=DEV)
    with pytest.raises(native.Kp1Error, match="KL gate"):
        k.anchor_loss_grad(w.buf["obs"], w.sels[0], w.n, teacher, loss_weight=1.0, grad_out=run.grad, loss_out=loss)
    with pytest.raises(native.Kp1Error, match="KL gate"):
        k.anchor_adam_step(run.p, run.grad, run.m, run.v, lr=1e-3, eps=1e-5, max_grad_norm=0.5, step=0)
    with pytest.raises(native.Kp1Error, match="KL gate"):
        k.set_actor_extra_steps(1)
    assert _same(run.state(), before) and k.kl_gate_read()[1] == [1]
    k.close()
    fresh_k.close()


def test_population_replicas_stop_independently():
    """K = 3 with targets [none, a, b]: replica 1 stops in the first minibatch (stop_index 0, no step at all), replica 2 later, replica 0
    never; every replica is bit-equal to a K = 1 gated handle with its target, and the step counts are per replica"""
    K, pairs = 3, 4
    w = _World(64, 64, pairs=pairs)
    sels = [[S.selection(S.TOTAL, w.n, 100 * r + i).to(DEV) for i in range(pairs)] for r in range(K)]
    traces = [_twin_trace(w, sels[r]) for r in range(K)]
    late = _first_new_maximum(traces[2], (2, 3))
    targets = [None, _threshold(traces[1], 0) / 1.5, _threshold(traces[2], late) / 1.5]
    kp = w.handle(targets, replicas=K)
    pop = _Run(w, kp, replicas=K)
    for i in range(pairs):
        pop.pair(torch.stack([sels[r][i] for r in range(K)]).contiguous())
    rec, steps = kp.kl_gate_read()
    assert steps == [pairs, 0, late]
    assert [r["stopped"] for r in rec] == [0, 1, 1] and [r["stop_index"] for r in rec] == [0, 0, late]
    assert [r["n_counted"] for r in rec] == [pairs, 1, late + 1] and [r["n_seen"] for r in rec] == [pairs] * K
    assert rec[1]["stop_kl"] == traces[1][0] and rec[2]["stop_kl"] == traces[2][late]
    P = w.flat0.numel()
    for r in range(K):
        k1 = w.handle([targets[r]])
        one = _Run(w, k1)
        for i in range(pairs):
            one.pair(sels[r][i])
        rec1, steps1 = k1.kl_gate_read()
        assert steps1 == [steps[r]] and rec1[0] == rec[r], r
        sl = slice(r * P, (r + 1) * P)
        assert _same([pop.p[sl], pop.m[sl], pop.v[sl], pop.stats[4 * r:4 * r + 4]], one.state() + [one.stats]), r
        k1.close()
    assert torch.equal(pop.p[P:2 * P], w.flat0) and not torch.equal(pop.p[:P], w.flat0)
    with pytest.raises(ValueError, match="differ"):
        kp.set_kl_gate(None)      # one shared count cannot hold 4, 0 and `late`
    assert kp.kl_gate and kp.kl_gate_read()[1] == steps
    kp.set_step_count(7)          # sets every replica's
    assert kp.kl_gate_read()[1] == [7] * K
    kp.set_kl_gate(None)
    assert not kp.kl_gate
    kp.close()


# ================================================================================================ trainer level
N_ENVS, N_STEPS, N_EPOCHS, N_MB = 16, 64, 4, 4
LR = 3e-4


def _env_cfg():
    from rl_brain_trainer_amd import config as kcfg

    return kcfg.to_env_config(kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"))


def _pcfg(seed: int = 7, **kw):
    from rl_brain_trainer_amd.ppo import PPOConfig

    return PPOConfig(n_steps=N_STEPS, batch_size=256, n_epochs=N_EPOCHS, hidden=64, learning_rate=LR, ent_coef=1e-3, seed=seed, **kw)


def _trainer(env_cfg, cfg, **kw):
    from rl_brain_trainer_amd.ppo import PPO
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    return PPO(ArmKinematicVecEnv(env_cfg, N_ENVS, seed=cfg.seed), cfg, **kw)


def _sb3_train(ppo, threshold: float | None) -> dict:
    """stable_baselines3/ppo/ppo.py train() restated over the eager minibatch calls of an UNGATED trainer: the loss terms of a minibatch are
    logged, then its approx_kl is tested, and only then is the optimiser step taken.  Each minibatch's loss_grad runs twice -- once into a
    zeroed stats_out (the float the device compares) and once into the accumulated one (the device's own sum) -- so the Adam launch takes
    its count from the host here."""
    cfg, mlp = ppo.cfg, ppo._mlp
    T, total = cfg.n_steps, cfg.n_steps * ppo.n_envs
    obs = ppo.obs_buf[:T].view(total, ppo.obs_w)
    act, old_logp, adv, ret = ppo.act_buf.view(total, 7), ppo.logp_buf.view(total), ppo.adv_buf.view(total), ppo.ret_buf.view(total)
    kw = dict(clip_range=cfg.clip_range, ent_coef=cfg.ent_coef, vf_coef=cfg.vf_coef, grad_out=ppo.grad, normalize=cfg.normalize_advantage)
    acc = torch.zeros(4, device=ppo.device)
    out = {"trace": [], "steps": 0, "n_updates": 0, "n_counted": 0, "stop": None}
    continue_training = True
    for epoch in range(cfg.n_epochs):
        ppo._draw_perm(0)
        perm = ppo.perm[0]
        mb_stats = ppo._epoch_adv_stats(adv, perm, total, cfg.batch_size)
        for i, start in enumerate(range(0, total, cfg.batch_size)):
            idx = perm[start:start + cfg.batch_size]
            n = int(idx.numel())
            one = torch.zeros(4, device=ppo.device)
            mlp.loss_grad(obs, idx, n, act, old_logp, adv, ret, inv_count=1.0 / n, stats_out=one, adv_stats=mb_stats[i], **kw)
            mlp.loss_grad(obs, idx, n, act, old_logp, adv, ret, inv_count=1.0 / n, stats_out=acc, adv_stats=mb_stats[i], **kw)
            out["n_counted"] += 1
            kl = float(one[3])
            out["trace"].append(kl)
            if threshold is not None and kl > threshold:
                continue_training = False
                out["stop"] = (epoch, i, kl)
                break
            mlp.set_step_count(out["steps"] + 1)
            mlp.adam_step(ppo.policy.flat, ppo.grad, ppo.adam_m, ppo.adam_v, lr=cfg.learning_rate, eps=cfg.adam_eps,
                          max_grad_norm=cfg.max_grad_norm, step=0, fused_norm=True)
            out["steps"] += 1
        out["n_updates"] += 1
        if not continue_training:
            break
    out["means"] = (acc / out["n_counted"]).tolist()
    out["state"] = [t.clone() for t in (ppo.policy.flat, ppo.adam_m, ppo.adam_v)]
    return out


@pytest.fixture(scope="module")
def twin():
    """the ungated twin's full trace, the stop position inside epoch 1 it allows, and SB3's loop with that threshold"""
    env_cfg = _env_cfg()
    a = _trainer(env_cfg, _pcfg(), use_graphs=False)
    a.collect_rollouts()
    full = _sb3_train(a, None)
    a.env.close()
    trace = full["trace"]
    assert len(trace) == N_EPOCHS * N_MB and full["steps"] == len(trace)
    assert max(trace[N_MB:2 * N_MB]) > max(trace[:N_MB]) > 0.0, f"the twin's KL trace does not rise from epoch 0 to epoch 1: {trace}"
    pos = _first_new_maximum(trace, (N_MB + 1, N_MB + 2))      # mid-epoch of epoch 1
    thr = _threshold(trace, pos)
    b = _trainer(env_cfg, _pcfg(), use_graphs=False)
    b.collect_rollouts()
    ref = _sb3_train(b, thr)
    b.env.close()
    assert ref["stop"][:2] == (1, pos - N_MB) and ref["stop"][2] == trace[pos] and ref["steps"] == pos and ref["n_updates"] == 2
    return {"env_cfg": env_cfg, "full": full, "trace": trace, "pos": pos, "thr": thr, "target": thr / 1.5, "ref": ref}


def _gated_iteration(twin, *, use_graphs: bool, **kw):
    ppo = _trainer(twin["env_cfg"], _pcfg(target_kl=twin["target"]), use_graphs=use_graphs, **kw)
    ppo.collect_rollouts()
    ppo.train()
    return ppo


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
def test_trainer_stops_where_sb3_breaks(twin, use_graphs):
    """a gated train() against SB3's control flow restated in Python, bit for bit: parameters, Adam moments, step count, the logged means
    and _n_updates -- as eager launches and (the warm-up epoch aside) as replays of the captured epoch"""
    ref, pos = twin["ref"], twin["pos"]
    ppo = _gated_iteration(twin, use_graphs=use_graphs)
    assert ("kl_gate", (twin["target"],)) in ppo._epoch_key() and ppo._mlp.kl_gate
    assert (ppo._epoch_graph is not None) == use_graphs
    stats = ppo.last_stats
    assert _same([ppo.policy.flat, ppo.adam_m, ppo.adam_v], ref["state"])
    assert ppo.adam_step_count() == ref["steps"] == pos and ppo.adam_t == pos and ppo.n_updates() == ref["n_updates"] == 2
    assert [stats[k] for k in ("policy_loss", "value_loss", "entropy", "approx_kl")] == ref["means"]
    assert stats["n_updates"] == ref["n_counted"] == pos + 1
    want = {"early_stop": True, "stop_epoch": 1, "stop_minibatch": pos - N_MB, "stop_kl": twin["trace"][pos]}
    assert ppo.kl_stops() == [want] and {k: stats[k] for k in want} == want
    # the next iteration re-arms and trains: its first minibatch comes from a fresh rollout (KL ~ 0), so at least one step is taken
    ppo.collect_rollouts()
    ppo.train()
    stop2 = ppo.kl_stops()[0]
    assert ppo.adam_step_count() > pos and ppo.n_updates() == 2 + (stop2["stop_epoch"] + 1 if stop2["early_stop"] else N_EPOCHS)
    assert ppo.last_stats["n_updates"] >= 2
    ppo.env.close()


def test_a_trainer_without_a_target_is_the_parent(twin):
    """target_kl=None against a twin built without the field: no gate, the parent's graph key, the same bits -- which are also those of the
    restated loop run to its end"""
    from rl_brain_trainer_amd.ppo import PPOConfig

    cfg = PPOConfig(n_steps=N_STEPS, batch_size=256, n_epochs=N_EPOCHS, hidden=64, learning_rate=LR, ent_coef=1e-3, seed=7)
    runs = []
    for c in (_pcfg(target_kl=None), cfg):
        ppo = _trainer(twin["env_cfg"], c, use_graphs=True)
        ppo.collect_rollouts()
        ppo.train()
        assert ppo.kl_targets is None and not ppo._mlp.kl_gate
        key = ppo._epoch_key()
        assert len(key) == 11 and not any(isinstance(e, tuple) for e in key)
        assert ppo.adam_t == N_EPOCHS * N_MB and ppo.n_updates() == N_EPOCHS
        with pytest.raises(ValueError, match="no KL gate"):
            ppo._mlp.kl_gate_read()
        runs.append(([ppo.policy.flat.clone(), ppo.adam_m.clone(), ppo.adam_v.clone()], ppo.last_stats))
        ppo.env.close()
    assert _same(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert _same(runs[0][0], twin["full"]["state"])
    assert [runs[0][1][k] for k in ("policy_loss", "value_loss", "entropy", "approx_kl")] == twin["full"]["means"]
    assert "early_stop" not in runs[0][1]


def test_checkpoint_of_a_stopped_run(twin, tmp_path):
    from rl_brain_trainer_amd import checkpoint

    ppo = _gated_iteration(twin, use_graphs=True)
    path = checkpoint.save(tmp_path / "stopped", ppo, twin["env_cfg"])
    data = checkpoint.load_data(path)
    assert data["target_kl"] == twin["target"] and data["_n_updates"] == 2 and data["n_epochs"] == N_EPOCHS
    assert data["kp1_engine"]["adam_steps"] == twin["pos"]
    opt = checkpoint.load_optimizer_state_dict(path)
    assert {float(s["step"]) for s in opt["state"].values()} == {float(twin["pos"])}
    ppo.env.close()
    plain = _trainer(twin["env_cfg"], _pcfg(), use_graphs=False)
    assert checkpoint.load_data(checkpoint.save(tmp_path / "plain", plain, twin["env_cfg"]))["target_kl"] is None
    plain.env.close()


def test_monitor_reports_the_stop(twin, capsys):
    ppo = _gated_iteration(twin, use_graphs=True, monitor=True)
    loggers = ppo.make_loggers()
    capsys.readouterr()
    row = loggers[0].log(ppo.monitor_rows()[0], iteration=1, total_timesteps=ppo.num_timesteps)
    text = capsys.readouterr().out
    assert f"Early stopping at step 1 due to reaching max kl: {twin['trace'][twin['pos']]:.2f}" in text
    assert row["train/n_updates"] == 2 and row["train/approx_kl"] == ppo.last_stats["approx_kl"]
    ppo.collect_rollouts()
    ppo.train()
    stop2 = ppo.kl_stops()[0]
    row2 = loggers[0].log(ppo.monitor_rows()[0], iteration=2, total_timesteps=ppo.num_timesteps)
    assert row2["train/n_updates"] == 2 + (stop2["stop_epoch"] + 1 if stop2["early_stop"] else N_EPOCHS)      # the running total of epochs begun
    assert ("Early stopping" in capsys.readouterr().out) == stop2["early_stop"]
    ppo.env.close()
    ppo.monitor.close()


def test_approach_population_sweeps_target_kl(twin):
    """ApproachPopulationPPO, K = 2, overrides target_kl = [x, none]: each replica equals the single trainer of its seed and target"""
    from rl_brain_trainer_amd.population import ApproachPopulationPPO
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    seeds, targets = [7, 8], [twin["target"], None]
    penv = ArmKinematicPopulationVecEnv(twin["env_cfg"], seeds, N_ENVS)
    pop = ApproachPopulationPPO(seeds, _pcfg(), penv, overrides=[{"target_kl": t} for t in targets])
    assert pop.kl_targets == targets and pop.replica_names == [f"seed_7_target_kl_{twin['target']!r}", "seed_8_target_kl_none"]
    pop.collect_rollouts()
    pop.train()
    stops, rows = pop.kl_stops(), pop._stats_rows()
    assert stops[0]["early_stop"] and (stops[0]["stop_epoch"], stops[0]["stop_minibatch"]) == (1, twin["pos"] - N_MB) and not stops[1]["early_stop"]
    for k, (s, t) in enumerate(zip(seeds, targets)):
        single = _trainer(twin["env_cfg"], _pcfg(seed=s, target_kl=t), use_graphs=True)
        single.collect_rollouts()
        single.train()
        assert _same([pop.flat[k], pop.adam_m[k], pop.adam_v[k]], [single.policy.flat, single.adam_m, single.adam_v]), k
        one = single.last_stats
        assert all(rows[k][q] == one[q] for q in ("policy_loss", "value_loss", "entropy", "approx_kl", "n_updates")), (k, rows[k], one)
        assert pop.adam_step_count(k) == single.adam_step_count() and pop.n_updates(k) == single.n_updates()
        assert pop.replica(k).adam_t == single.adam_step_count() and pop.replica(k).cfg.target_kl == t
        single.env.close()
    assert pop.adam_step_count(0) == twin["pos"] and pop.adam_step_count(1) == N_EPOCHS * N_MB
    pop.close()
    penv.close()
