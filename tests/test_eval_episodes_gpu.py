"""The whole-episode evaluation kernel (kp1_eval_episodes: all env steps of a phase in one launch) and the host paths that take it, on the GPU.

The reference is always a second env handle driven by kp1_eval_step one step at a time to the episode limit + 1.  After each step the
reference keeps, for the rows that were alive BEFORE that step, a copy of the observation row, reward, done and every env.info() field:
each row's values at its own last step, which is what kp1_eval_episodes leaves (it does not step a finished row again).

Inputs.  E = 70 rows (tiles of 32, 32, 6) of workspace_expansion_bigtrain (96 steps) / dock_workspace_handoff_noop_ft_12env_raw (36 steps)
with the termination rewritten so that episodes end at different steps: terminate_on_success on, no dwell, no orientation clause, success
within 0.04 m.  Under the head-scaled policies about half of the rows come within 0.04 m at some step and the rest never do (they run to the
limit); rows 64.. (the whole last tile) start AT their goal and end at step 1 (one step moves the end effector by at most 0.02 m).  The
population case has n = 35 rows per replica (tiles of 32 and 3) and its rows 32.. start at their goal.  _check_exits asserts on the
reference's counters that the inputs do exercise the loop's exits.

The env step's fp32 sums and reward are not contraction-pinned, so these equalities also guard how the compiler fuses them in the episode
instantiations (kp1_eval_step.inc, ES_EPISODE_REREADS): a mismatch of one unit in the last place of reward or action_l2 in a few rows is
that, and _assert_equal_to_reference prints the figures before it asserts.

Refusals not reachable from Python on one device and therefore not covered: a hidden width other than 64 / 128 / 256 (no such handle can
be created), a third env mode, handles on different devices.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest
import torch

import eval_forms as F
from conftest import load_golden_config
from eval_forms import DEV, NAMES, READY, THR
from rl_brain_trainer_amd import evaluate as ev
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import ppo as P
from rl_brain_trainer_amd import workspace_coverage as wc
from rl_brain_trainer_amd.mlp import MlpKernels
from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

pytestmark = pytest.mark.gpu
E, K, N_POP = 70, 3, 35
SUCCESS_RADIUS = 0.04
INVALID, UNSUPPORTED = -1, -4


def _cfg(mode: str, early_ends: bool = True):
    cfg = load_golden_config("workspace_expansion_bigtrain" if mode == "approach" else "dock_workspace_handoff_noop_ft_12env_raw")
    if early_ends:
        t = cfg.c.termination
        t.terminate_on_success, t.success_dwell_steps, t.require_orientation, t.success_pos_threshold_m = 1, 0, 0, SUCCESS_RADIUS
    return cfg


@pytest.fixture(scope="module")
def handles():
    """name -> (MlpKernels, replicas): K = 1 handles of hidden 256 / 64 / 128 and a hidden-64 population of three"""
    pols = {"h256": P.InferencePolicy(F.state_dict(256, 21), device=DEV, max_batch=128),
            "h64": P.InferencePolicy(F.state_dict(64, 11), device=DEV, max_batch=128),
            "h128": P.InferencePolicy(F.state_dict(128, 11), device=DEV, max_batch=128)}
    rest = [P.InferencePolicy(F.state_dict(64, 11 + k), device=DEV, max_batch=128) for k in (1, 2)]
    pop = MlpKernels(64, DEV, max_batch=64, replicas=K)
    pop.pack(torch.stack([p.policy.flat for p in (pols["h64"], *rest)]).contiguous())
    out = {k: (v._mlp, 1) for k, v in pols.items()}
    out["pop64"] = (pop, K)
    out["_keep"] = (pols, rest)
    return out


@pytest.fixture(scope="module")
def suite():
    """70 explicit resets: 35 episodes each of two stages of workspace_expansion_bigtrain's curriculum-local suite"""
    return F.build_suite(_cfg("approach"), E // 2)


def _opts(suite, mode: str, n: int, reps: int = 1) -> dict:
    """rows [0, n) of the suite, those of the last (ragged) tile starting at their goal; tiled `reps` times"""
    o = {k: v[:n].copy() for k, v in suite.items()}
    if n > 32:
        o["initial_q"][n - n % 32:] = o["goal_q"][n - n % 32:]
    return {**{k: np.tile(v, (reps, 1)) for k, v in o.items()}, "policy_mode": mode}


def _env_snapshot(env) -> dict[str, torch.Tensor]:
    """obs / reward / done / every info field, cloned; the env axis is the FIRST of obs and the LAST of everything else"""
    return {"obs": env.obs.clone(), "reward": env.reward.clone(), "done": env.done.clone(), **{"info_" + k: v.clone() for k, v in env.info().items()}}


def _started(mlp, mode: str, stride: int, confirm: int, n: int, suite, reps: int = 1, active=None):
    """a freshly reset env of reps x n rows with kp1_eval_accumulate's step 0 made under the active mask"""
    L = native.load()
    env = F.make_env(_cfg(mode), reps * n, stride, _opts(suite, mode, n, reps))
    b = ev.EpisodeBuffers(reps * n, DEV, want_hand=True)
    thr = (C.c_double * 4)(*THR)
    active = F.forced_active_mask(reps * n) if active is None else active
    native.check(L.kp1_eval_accumulate(env._handle, C.byref(b.struct), None, None, F.ptr(active), 0, thr, confirm, F.stream()))
    return env, b, thr, active


_REFERENCES: dict[tuple, dict] = {}


def _reference(handles, name: str, mode: str, stride: int, confirm: int, n: int, suite, active_key: str = "mask") -> dict:
    """kp1_eval_step, steps 1 .. limit + 1, on a handle of its own; computed once per case and never changed afterwards"""
    key = (name, mode, stride, confirm, n, active_key)
    if key in _REFERENCES:
        return _REFERENCES[key]
    L = native.load()
    mlp, reps = handles[name]
    active = None
    if active_key == "tile1_off":
        active = F.forced_active_mask(reps * n)
        active[32:64] = 0
    env, b, thr, active = _started(mlp, mode, stride, confirm, n, suite, reps, active)
    post_reset = _env_snapshot(env)
    last = {k: v.clone() for k, v in post_reset.items()}
    limit = env.config.c.termination.max_episode_steps
    for step in range(1, limit + 2):
        alive = b.flags[0].bool().clone()                  # alive BEFORE this step
        native.check(L.kp1_eval_step(mlp._h, env._handle, F.ptr(env.obs), F.ptr(env.reward), F.ptr(env.done), C.byref(b.struct), step, thr, confirm, F.stream()))
        last["obs"][alive] = env.obs[alive]
        last["reward"][alive] = env.reward[alive]
        last["done"][alive] = env.done[alive]
        for k, v in env.info().items():
            last["info_" + k][..., alive] = v[..., alive]
    ref = {"bufs": F.snapshot(b), "last": last, "post_reset": post_reset, "active": active, "limit": limit, "rows": n, "reps": reps}
    env.close()
    _REFERENCES[key] = ref
    return ref


def _assert_equal_to_reference(env, b: ev.EpisodeBuffers, ref: dict, what) -> None:
    for k in NAMES:
        assert torch.equal(getattr(b, k), ref["bufs"][k]), (what, k)
    got = _env_snapshot(env)
    for k, v in ref["last"].items():
        if v.is_floating_point() and not torch.equal(got[k], v):      # the figures, before the assertion
            d = (got[k].double() - v.double()).abs()
            print(f"{what} {k}: {int((d > 0).sum())} of {d.numel()} elements differ, max |difference| {float(d.max()):.3e}, "
                  f"max relative {float((d / v.double().abs().clamp_min(1e-300)).max()):.3e}")
        assert torch.equal(got[k], v), (what, k)
    off = ref["active"] == 0
    assert bool(off.any()) or ref["rows"] == 1
    for k, v in ref["post_reset"].items():
        sel = (lambda t: t[off]) if k == "obs" else (lambda t: t[..., off])
        assert torch.equal(sel(got[k]), sel(v)), (what, "inactive rows", k)


def _episodes(handles, name, mode, stride, confirm, n, suite, segments, active=None):
    """kp1_eval_episodes over consecutive [first, last] segments on a fresh handle -> (env, buffers)"""
    L = native.load()
    mlp, reps = handles[name]
    env, b, thr, _ = _started(mlp, mode, stride, confirm, n, suite, reps, active)
    for first, last in segments:
        native.check(L.kp1_eval_episodes(mlp._h, env._handle, F.ptr(env.obs), F.ptr(env.reward), F.ptr(env.done), C.byref(b.struct), first, last, thr, confirm,
                                         F.stream()))
    return env, b


def _check_exits(ref: dict) -> None:
    """conditions on the INPUT (not tolerances), asserted on the reference's counters: the loop's exits are exercised"""
    steps, active, limit, n = ref["bufs"]["counters"][0].cpu().numpy(), ref["active"].cpu().numpy() != 0, ref["limit"], ref["rows"]
    assert int(ref["bufs"]["n_alive"]) == 0 and not bool(ref["bufs"]["flags"][0].any())
    assert (steps[~active] == 0).all()
    ran = steps[active]
    assert (ran < limit).any() and (ran == limit).any()                    # some episode ends before the limit, some runs to it
    tiles = []
    for r in range(ref["reps"]):
        for lo in range(0, n, 32):
            s = steps[r * n + lo:r * n + min(lo + 32, n)]
            tiles.append(s[s > 0])
    assert any(len(set(t.tolist())) >= 2 for t in tiles)                   # a tile whose rows end at different steps
    lasts = [int(t.max()) for t in tiles if len(t)]
    assert max(lasts) - min(lasts) >= 2                                    # a tile's last episode ends well before another tile's


# ---------------------------------------------------------------------------------------------------------------- 1. parity
def _parity(handles, suite, name, mode, stride, confirm, n, check_exits):
    ref = _reference(handles, name, mode, stride, confirm, n, suite)
    if check_exits:
        _check_exits(ref)
    env, b = _episodes(handles, name, mode, stride, confirm, n, suite, [(1, ref["limit"] + 1)])
    _assert_equal_to_reference(env, b, ref, (name, mode, stride, confirm, n))
    env.close()


@pytest.mark.parametrize("confirm", [0, 2])
@pytest.mark.parametrize("stride", [56, 64])
@pytest.mark.parametrize("mode", ["approach", "dock"])
@pytest.mark.parametrize("name", ["h256", "h64", "h128"])
def test_one_call_equals_the_step_sequence(handles, suite, name, mode, stride, confirm):
    """one kp1_eval_episodes(1, limit + 1) call: every kp1_eval_buffers array and n_alive, and per row the observation, reward, done and info
    fields of the row's own last step; rows with active == 0 keep their post-reset values"""
    _parity(handles, suite, name, mode, stride, confirm, E, True)


@pytest.mark.parametrize("confirm", [0, 2])
@pytest.mark.parametrize("stride", [56, 64])
@pytest.mark.parametrize("mode", ["approach", "dock"])
def test_population_one_call_equals_the_step_sequence(handles, suite, mode, stride, confirm):
    """a hidden-64 population of three, 35 rows per replica (tiles of 32 and 3 in each replica)"""
    _parity(handles, suite, "pop64", mode, stride, confirm, N_POP, True)


@pytest.mark.parametrize("n", [1, 32, 33])
@pytest.mark.parametrize("name", ["h256", "h64"])
def test_row_counts(handles, suite, name, n):
    """one row, exactly one tile, one tile and one row"""
    _parity(handles, suite, name, "approach", 56, 2, n, False)


# ---------------------------------------------------------------------------------------------------------------- 2. segments
@pytest.mark.parametrize("mode", ["approach", "dock"])
@pytest.mark.parametrize("name", ["h256", "h128", "pop64"])
def test_segments_equal_the_single_call(handles, suite, name, mode):
    """(1, 3) then (4, limit + 1) leaves what the single call leaves; a further call after everything has ended changes nothing"""
    n = N_POP if name == "pop64" else E
    ref = _reference(handles, name, mode, 64, 2, n, suite)
    limit = ref["limit"]
    env, b = _episodes(handles, name, mode, 64, 2, n, suite, [(1, 3), (4, limit + 1)])
    _assert_equal_to_reference(env, b, ref, (name, mode, "segments"))
    mlp = handles[name][0]
    thr = (C.c_double * 4)(*THR)
    native.check(native.load().kp1_eval_episodes(mlp._h, env._handle, F.ptr(env.obs), F.ptr(env.reward), F.ptr(env.done), C.byref(b.struct), limit + 2, limit + 9,
                                                 thr, 2, F.stream()))
    assert int(b.n_alive) == 0
    _assert_equal_to_reference(env, b, ref, (name, mode, "after the end"))
    env.close()


@pytest.mark.parametrize("name", ["h256", "h64"])
def test_a_switched_off_tile_is_untouched(handles, suite, name):
    """rows 32 .. 63 inactive: that tile's env rows, observations and buffers are what the reset and step 0 left"""
    ref = _reference(handles, name, "approach", 56, 2, E, suite, active_key="tile1_off")
    assert not bool(ref["active"][32:64].any()) and bool(ref["active"][:32].any())
    env, b = _episodes(handles, name, "approach", 56, 2, E, suite, [(1, ref["limit"] + 1)], active=ref["active"])
    _assert_equal_to_reference(env, b, ref, (name, "tile off"))
    got = _env_snapshot(env)
    for k, v in ref["post_reset"].items():
        assert torch.equal(got[k][32:64] if k == "obs" else got[k][..., 32:64], v[32:64] if k == "obs" else v[..., 32:64]), k
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3. host
def _count_library_calls(monkeypatch):
    L = native.load()
    calls = {"step": 0, "episodes": 0}

    class Counting:
        def __getattr__(self, name):
            f = getattr(L, name)
            if name == "kp1_eval_step":
                def g(*a):
                    calls["step"] += 1
                    return f(*a)
                return g
            if name == "kp1_eval_episodes":
                def g(*a):
                    calls["episodes"] += 1
                    return f(*a)
                return g
            return f

    monkeypatch.setattr(native, "load", lambda: Counting())
    return calls


def _run_fused(handles, suite, name, mode, confirm, whole, max_steps=None):
    mlp, reps = handles[name]
    n = N_POP if reps > 1 else E
    env = ArmKinematicVecEnv(_cfg(mode), reps * n, seed=3)
    env.set_obs_stride(64)
    out = ev.run_episodes_fused(env, mlp, _opts(suite, mode, n, reps), ready_cfg=READY, handoff_confirm_steps=confirm,
                                active=F.forced_active_mask(reps * n).bool(), max_steps=max_steps, whole_episodes=whole)
    env.close()
    return out


def _assert_dicts_equal(a, b, what) -> None:
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert set(a) == set(b), what
    for k in b:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("mode,confirm", [("approach", 2), ("dock", None)])
@pytest.mark.parametrize("name", ["h256", "h64", "pop64"])
def test_run_episodes_fused_whole_episodes_equals_per_step(monkeypatch, handles, suite, name, mode, confirm):
    calls = _count_library_calls(monkeypatch)
    res, hand = _run_fused(handles, suite, name, mode, confirm, True)
    limit = _cfg(mode).c.termination.max_episode_steps + 1
    assert calls["step"] == 0 and 1 <= calls["episodes"] <= math.ceil(limit / native.EVAL_EPISODES_MAX_STEPS)
    ref, ref_hand = _run_fused(handles, suite, name, mode, confirm, False)
    assert calls["step"] >= 2
    _assert_dicts_equal(res, ref, "final")
    _assert_dicts_equal(hand, ref_hand, "handoff")
    assert int(ref["step_count"].max()) >= 2 and len(set(ref["step_count"].tolist())) >= 3


def test_a_limit_above_the_cap_is_split(monkeypatch, handles, suite):
    """a cap of 5 steps per call (monkeypatched) on a 97-step limit: consecutive calls until no episode is alive; and a max_steps above the
    library's 256 with the real cap: two calls at the most, the second skipped when nothing is alive"""
    ref, ref_hand = _run_fused(handles, suite, "h256", "approach", 2, False)
    calls = _count_library_calls(monkeypatch)
    monkeypatch.setattr(ev, "_EPISODES_CAP", 5)
    res, hand = _run_fused(handles, suite, "h256", "approach", 2, True)
    assert calls["step"] == 0 and calls["episodes"] == math.ceil(97 / 5)
    _assert_dicts_equal(res, ref, "final")
    _assert_dicts_equal(hand, ref_hand, "handoff")
    monkeypatch.setattr(ev, "_EPISODES_CAP", native.EVAL_EPISODES_MAX_STEPS)
    calls["episodes"] = 0
    res, hand = _run_fused(handles, suite, "h256", "approach", 2, True, max_steps=300)
    assert calls["episodes"] == 1          # every episode is truncated at step 96: n_alive reads 0 before the second call
    _assert_dicts_equal(res, ref, "final")


def _servo(obs):
    return torch.tanh(obs[:, :7])


def test_evaluators_whole_episodes_equal_per_step(tmp_path, monkeypatch, handles):
    """evaluate_workspace_expansion and _run_pairs_columns: equal payloads / columns, no kp1_eval_step call, at most one kp1_eval_episodes
    call per phase; True on a phase without a covered handle raises"""
    pols, rest = handles["_keep"]
    calls = _count_library_calls(monkeypatch)
    acfg, fcfg = _cfg("approach", False), _cfg("dock", False)
    kw = dict(approach_policy=pols["h256"].predict, finisher_policy=rest[0], approach_cfg=acfg, finisher_cfg=fcfg, episodes=4, seed=700001,
              stage_indices=[0, 3], handoff_confirm_steps=0, gate_config={"score_stage_index": 3})
    got = ev.evaluate_workspace_expansion(artifact_root=tmp_path / "whole", whole_episodes=True, **kw)
    assert calls == {"step": 0, "episodes": 2}
    ref = ev.evaluate_workspace_expansion(artifact_root=tmp_path / "steps", whole_episodes=False, **kw)
    assert calls["episodes"] == 2 and calls["step"] > 2
    assert got == ref and len(got["target_rows"]) == 8
    with pytest.raises(ValueError, match="whole_episodes=True: the Approach phase"):
        ev.evaluate_workspace_expansion(**{**kw, "approach_policy": _servo}, whole_episodes=True)
    with pytest.raises(ValueError, match="whole_episodes=True"):
        ev.evaluate_workspace_expansion(one_launch=False, whole_episodes=True, **kw)

    cfg = load_golden_config("workspace_full_coverage_randomstart_overnight")
    fk = wc._device_fk(0)
    targets, _ = wc.generate_workspace_target_map(cfg, seed=940002, stage_samples_per_stage=8, random_samples=64, fk=fk)
    starts, _ = wc.generate_workspace_start_state_map(cfg, seed=940003, stage_samples_per_stage=4, random_samples=64, fk=fk)
    pairs, _ = wc.build_pair_sampler_summary(starts=starts, targets=targets, seed=940004, pair_count=96)
    common = dict(pairs=pairs, starts_by_id={r["start_id"]: r for r in starts}, targets_by_id={r["target_id"]: r for r in targets},
                  approach_policy=pols["h256"].predict, approach_cfg=cfg, finisher_policy=pols["h128"].predict, finisher_cfg=fcfg,
                  handoff_confirm_steps=0, device=0, obs_stride=64, seed=760001, first_env_id=96)
    calls.update(step=0, episodes=0)
    got = wc._run_pairs_columns(whole_episodes=True, **common)
    assert calls["step"] == 0 and 1 <= calls["episodes"] <= 2 * math.ceil((cfg.c.termination.max_episode_steps + 1) / native.EVAL_EPISODES_MAX_STEPS)
    ref = wc._run_pairs_columns(whole_episodes=False, **common)
    assert got.shape == (96, len(wc._COLS)) and torch.equal(got, ref)


def test_population_evaluator_whole_episodes_equals_per_step(monkeypatch):
    from rl_brain_trainer_amd import config as kcfg
    from rl_brain_trainer_amd.population import ApproachPopulationPPO
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    env_cfg = kcfg.to_env_config(kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"))
    seeds = [7, 8, 9]
    penv = ArmKinematicPopulationVecEnv(env_cfg, seeds, 16)
    pop = ApproachPopulationPPO(seeds, P.PPOConfig(n_steps=32, batch_size=128, n_epochs=2, hidden=64, learning_rate=3e-3), penv)
    pop.learn(pop.n_envs * pop.cfg.n_steps)
    fin = P.InferencePolicy(F.state_dict(64, 5), device=DEV)
    kw = dict(population=pop, finisher_policy=fin, approach_cfg=env_cfg, finisher_cfg=_cfg("dock", False), episodes=4, seed=700001, stage_indices=[0, 3],
              handoff_confirm_steps=0, gate_config={"score_stage_index": 3})
    calls = _count_library_calls(monkeypatch)
    got = ev.evaluate_workspace_expansion_population(whole_episodes=True, **kw)
    assert calls == {"step": 0, "episodes": 2}
    ref = ev.evaluate_workspace_expansion_population(whole_episodes=False, **kw)
    assert got == ref and len(got) == 3 and got[0]["target_rows"] != got[1]["target_rows"]
    pop.close()
    penv.close()


def test_evaluate_dock_whole_episodes_equals_per_step():
    from rl_brain_trainer_amd import train_dock

    env = ArmKinematicVecEnv(_cfg("dock", False), 64, seed=11)
    ppo = P.PPO(env, P.PPOConfig(n_steps=4, batch_size=256, n_epochs=1, hidden=256, seed=11), use_graphs=False)
    ppo.policy.views["action_net.weight"].mul_(250.0)
    ppo._mlp.pack(ppo.policy.flat)
    kw = dict(episodes=70, seed=10_011, device=0)
    got = train_dock.evaluate_dock(ppo, _cfg("dock", False), whole_episodes=True, **kw)
    assert got == train_dock.evaluate_dock(ppo, _cfg("dock", False), whole_episodes=False, **kw) and got["mean_episode_length"] >= 2.0
    with pytest.raises(ValueError, match="whole_episodes=True: the dock phase"):
        train_dock.evaluate_dock(ppo, _cfg("dock", False), one_launch=False, whole_episodes=True, **kw)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4. training handle
_TRAIN_EVAL_KW = dict(finisher_policy=None, finisher_cfg=None, episodes=4, seed=700001, stage_indices=[0, 3], handoff_confirm_steps=2, whole_episodes=True)


def test_whole_episode_evaluation_on_the_training_handle():
    """a 2x256 PPO with graphs on: [iteration, whole-episode evaluation through ppo.predict, iteration] leaves the parameters of
    [iteration, iteration], and the evaluation equals the one through a fresh InferencePolicy of the same weights"""
    out = []
    for evaluate in (True, False):
        ppo, env = F.trained_ppo(_cfg("approach", False))
        if evaluate:
            assert ev.policy_mlp(ppo.predict) is ppo._mlp
            got = ev.evaluate_workspace_expansion(approach_policy=ppo.predict, approach_cfg=_cfg("approach", False), obs_stride=ppo.obs_w, **_TRAIN_EVAL_KW)
            fresh = P.InferencePolicy({k: v.clone() for k, v in ppo.policy.state_dict().items()}, device=DEV)
            assert got == ev.evaluate_workspace_expansion(approach_policy=fresh.predict, approach_cfg=_cfg("approach", False), obs_stride=ppo.obs_w,
                                                          **_TRAIN_EVAL_KW)
        ppo.learn(256 * 8)
        torch.cuda.synchronize()
        out.append((ppo.policy.flat.clone(), ppo.adam_m.clone(), ppo.adam_v.clone(), ppo.obs_buf.clone()))
        env.close()
    assert all(torch.equal(x, y) for x, y in zip(*out))


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def _refused(mlp_h, env, status: int, text: str, first: int = 1, last: int = 4, mutate=None) -> None:
    """kp1_eval_episodes refuses with `status` and `text` in kp1_last_error and launches nothing: no buffer, observation or env field changes"""
    L = native.load()
    b = ev.EpisodeBuffers(env.n_envs, DEV, want_hand=True)
    for k in NAMES:
        getattr(b, k).fill_(7)
    args = [mlp_h, env._handle, F.ptr(env.obs), F.ptr(env.reward), F.ptr(env.done), C.byref(b.struct)]
    if mutate is not None:
        mutate(args, b.struct)
    before = _env_snapshot(env)
    rc = L.kp1_eval_episodes(*args, first, last, None, 0, F.stream())
    assert rc == status, (rc, L.kp1_last_error())
    assert text in L.kp1_last_error().decode(), L.kp1_last_error()
    torch.cuda.synchronize()
    for k in NAMES:
        assert bool((getattr(b, k) == 7).all()), k
    after = _env_snapshot(env)
    assert all(torch.equal(after[k], v) for k, v in before.items())


def test_refusals(handles, suite):
    opts = _opts(suite, "approach", 8)
    cfg = _cfg("approach")
    env = F.make_env(cfg, 8, 56, opts)
    h256, h64, pop = handles["h256"][0], handles["h64"][0], handles["pop64"][0]
    for mlp in (h256, h64):
        # the three of kp1_eval_episodes
        _refused(mlp._h, env, INVALID, "first_step must be at least 1", first=0)
        _refused(mlp._h, env, INVALID, "last_step is below first_step", first=5, last=4)
        _refused(mlp._h, env, INVALID, "at most KP1_EVAL_EPISODES_MAX_STEPS (256)", first=2, last=258)
        # kp1_eval_step's, with its texts
        for slot in range(5):
            _refused(mlp._h, env, INVALID, "NULL argument to kp1_eval_step", mutate=lambda a, b, s=slot: a.__setitem__(s, None))
        _refused(mlp._h, env, INVALID, "NULL argument to kp1_eval_step", mutate=lambda a, b: a.__setitem__(5, None))
        for field in ("metrics", "counters", "flags", "state", "n_alive"):
            _refused(mlp._h, env, INVALID, "kp1_eval_step: NULL buffer", mutate=lambda a, b, f=field: setattr(b, f, None))
        for field in ("hand_step", "hand_success", "hand_state"):
            _refused(mlp._h, env, INVALID, "incomplete handoff buffers", mutate=lambda a, b, f=field: setattr(b, f, None))
    _refused(pop._h, env, INVALID, "multiple of the handle's replica count")          # 8 envs, three replicas
    off = MlpKernels(256, DEV, max_batch=64)
    off.pack(handles["_keep"][0]["h256"].policy.flat)
    off.set_fused(False)
    _refused(off._h, env, UNSUPPORTED, "needs the tile kernels")
    off.close()
    wide = MlpKernels(256, DEV, max_batch=64, obs_dim=80)
    _refused(wide._h, env, UNSUPPORTED, "56-float observation")
    wide.close()
    stage = torch.zeros(1, dtype=torch.int32, device=DEV)
    native.check(native.load().kp1_bind_stage_ptr(env._handle, F.ptr(stage)))
    _refused(h256._h, env, UNSUPPORTED, "bound to a curriculum tracker")
    env.close()
    env64 = F.make_env(cfg, 8, 56, opts, real="f64")
    _refused(h256._h, env64, UNSUPPORTED, "fp32 handle")
    env64.close()
    comps = F.make_env(cfg, 8, 56, opts, reward_components=True)
    _refused(h64._h, comps, UNSUPPORTED, "reward components")
    comps.close()
