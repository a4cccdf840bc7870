"""The env handle's control surface (include/kp1.h beyond step / reset) against the fp64 oracle: reset options, set_state / get_state /
observe, snapshot / restore and the four setters that rewrite what the next launch reads.  Helpers, option table and comparison rules are
in tests/env_control.py; tests/test_env_control_cpu.py pins the oracle side.  Every test runs N = 130 envs: three 64-lane workgroups, the
last of which holds two lanes.

Two points where handle and reference differ by construction are pinned here (DESIGN.md has the reasoning):
- Stage index of an episode started with ``initial_q``: no stage is sampled, handle and oracle report the env's own curriculum stage --
  what the reference's info["curriculum_stage_index"] holds for it.
- Scope of the policy mode: the handle keeps ONE mode for all envs.  A ``policy_mode`` override stays in force at the auto-resets inside
  kp1_step and reaches the envs a mask leaves out, until the next ``reset`` without the option; the reference keeps the mode per env and
  returns to the config's mode at every reset without options.  No shipped caller steps with auto-reset under a differing override.

Each test prints its worst observed errors next to their bounds (``ENV_CONTROL {...}``, shown with ``-s``).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import env_control as ec
from conftest import load_golden_config
from oracle import oracle as orc
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import finisher_tools as ft
from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv
from test_env_parity_gpu import _two_float

pytestmark = pytest.mark.gpu

N = ec.N_ENVS
APPROACH, DOCK, SHORT_DOCK = "approach_default", "dock_workspace_handoff_noop_ft_12env_raw", "fuzz3_dock"
STAGE = {APPROACH: 3, DOCK: 0, SHORT_DOCK: 0}
SEED = 806
MODE_FLAG = kcfg.OBS_LAYOUT["mode_flag"][0]
MODE_COLUMN = {"approach": MODE_FLAG, "dock": MODE_FLAG + 1}


def _pair(name: str, real: str, *, seed: int = SEED, stage: int | None = None):
    cfg = load_golden_config(name)
    stage = STAGE[name] if stage is None else stage
    env = ArmKinematicVecEnv(cfg, N, seed=seed, real=real)
    env.set_curriculum_stage(stage)
    return cfg, env, orc.OracleVecEnv(cfg, N, seed0=seed, stage=stage)


def _actions(env, a: np.ndarray) -> torch.Tensor:
    return torch.tensor(a, dtype=env.dtype, device="cuda")


def _assert_mode(obs: torch.Tensor | np.ndarray, mode: str, rows=None, ctx: str = "") -> None:
    o = obs.cpu().numpy() if isinstance(obs, torch.Tensor) else obs
    o = o if rows is None else o[rows]
    assert np.all(o[:, MODE_COLUMN[mode]] == 1.0) and np.all(o[:, MODE_COLUMN[ec.other_mode(mode)]] == 0.0), f"{ctx}: mode flag is not {mode}"


# ============================================================================== reset options
@pytest.mark.parametrize("masked", [False, True], ids=["full", "masked"])
@pytest.mark.parametrize("real", ["f64", "f32"])
@pytest.mark.parametrize("name", [APPROACH, DOCK])
def test_reset_options_table(name, real, masked):
    """Every row of the option table, one after the other on one handle / oracle pair (so each row starts from the RNG words and the dirty
    counters the rows before it left): state, entry metrics, first observation, RNG words, stage index and the info norms after the reset.
    Masked: envs outside the mask keep every real, int and RNG word.  Full, f64: the step that follows each reset is compared too -- it is
    the first step of an episode handed over with non-zero dq and prev_action."""
    cfg, env, ora = _pair(name, real)
    stats = ec.Stats()
    v = ec.draw_options(cfg)
    mask = ec.reset_mask() if masked else None
    mask_t = torch.tensor(mask, device="cuda") if masked else None
    sel = mask.astype(bool) if masked else None
    ec.compare_obs(env.reset().cpu().numpy(), ec.reset(ora), real, stats, ctx="first reset")
    arng = np.random.default_rng(3)
    reached = set()
    for row in ec.option_table(cfg.mode_name):
        ctx = f"{name} {real} {row.name}"
        a = arng.uniform(-1.0, 1.0, size=(N, 7)).astype(np.float32).astype(np.float64)
        og, rg, dg = env.step(_actions(env, a), auto_reset=False)                # dirty counters, a moved state
        oo, ro, do, _ = ec.oracle_step(ora, a, auto_reset=False)
        if real == "f64" and not masked:
            assert np.array_equal(dg.cpu().numpy(), do), f"{ctx}: done bytes of the step before"
            stats.within("f64 step reward", np.abs(rg.cpu().numpy() - ro), ec.F64_REWARD_TOL, ctx)
            stats.within("f64 step observation", np.abs(og.cpu().numpy() - oo), ec.F64_OBS_TOL, ctx)
        before = ec.handle_arrays(env) if masked else None
        assert before is None or before["step_count"].min() > 0
        opts = ec.options_of(row, v)
        obs = env.reset(options=opts, mask=mask_t).cpu().numpy()
        obs_o = ec.reset(ora, opts, mask)
        h = ec.compare_state(env, ora, real, stats, rows=sel, ctx=ctx)
        ec.compare_obs(obs, obs_o, real, stats, rows=sel, ctx=ctx, name="reset observation")
        _assert_mode(obs, row.mode or cfg.mode_name, sel, ctx)
        if masked:
            ec.assert_same_words(before, h, rows=~sel, ctx=f"{ctx}: env outside the mask")
        if "initial_q" in row.keys:      # no stage is sampled: the episode's stage is the handle's own
            picked = h["stage_index"] if sel is None else h["stage_index"][sel]
            assert np.all(picked == env.get_curriculum_stage()), ctx
            assert env.get_curriculum_stage() == (STAGE[name] if cfg.c.curriculum_enabled else 0)
        reached.add((row.keys, row.mode))
    assert len(reached) == 96
    stats.report(f"test_reset_options_table[{name}-{real}-{'masked' if masked else 'full'}]")
    env.close()


@pytest.mark.parametrize("real", ["f64", "f32"])
def test_reset_options_broadcast_rows_and_errors(real):
    """1-D option rows are broadcast to every env; a wrong shape and an unknown policy_mode raise ValueError before anything is launched"""
    cfg, env, ora = _pair(APPROACH, real)
    stats = ec.Stats()
    v = ec.draw_options(cfg)
    env.reset()
    ec.reset(ora)
    for keys, r in ((ec.OPTION_KEYS, 0), (("initial_q",), 5), (("goal_pose6", "initial_dq"), 2), (("goal_q", "initial_prev_action"), 1)):
        opts = {k: v[k][r] for k in keys}
        assert all(o.ndim == 1 for o in opts.values())
        obs = env.reset(options=opts).cpu().numpy()
        ec.reset(ora, opts)
        ec.compare_state(env, ora, real, stats, ctx=f"broadcast {keys}")
        ec.compare_obs(obs, ora.obs, real, stats, ctx=f"broadcast {keys}", name="reset observation")
        st = env.get_state()
        if "initial_dq" in keys:
            assert np.all(st["dq"] == st["dq"][0])
    before = ec.handle_arrays(env)
    obs_before = env.obs.clone()
    for bad in ({"initial_q": np.zeros((N, 6))}, {"goal_pose6": np.zeros((N, 7))}, {"initial_dq": np.zeros((N - 1, 7))}, {"goal_q": np.zeros(6)},
                {"initial_q": v["initial_q"], "policy_mode": "bridge_typo"}, {"policy_mode": "dock_coarse"}):
        with pytest.raises(ValueError):
            env.reset(options=bad)
        with pytest.raises(ValueError):
            env.reset(options=bad, mask=torch.tensor(ec.reset_mask(), device="cuda"))
    ec.assert_same_words(before, ec.handle_arrays(env), ctx="after the refused resets")
    assert torch.equal(obs_before, env.obs)
    stats.report(f"test_reset_options_broadcast_rows_and_errors[{real}]")
    env.close()


# ============================================================================== set_state / get_state / observe
@pytest.mark.parametrize("stride", [56, 64])
@pytest.mark.parametrize("real", ["f64", "f32"])
def test_set_state_get_state_observe(real, stride):
    """kp1_set_state mid-episode: all five fields, then each alone, with and without the entry-metric capture; get_state, info() and
    current_observation() against the oracle counterpart at both observation pitches; then 20 steps from the placed state."""
    cfg, env, ora = _pair(APPROACH, real)
    if stride != 56:
        env.set_obs_stride(stride)
    stats = ec.Stats()
    run = ec.Lockstep(env, ora, cfg, real, stats)
    run.start()
    run.run(5)
    draws = [ec.draw_options(cfg, seed=s) for s in (11, 12, 13)]

    def place(ctx, capture, **fields):
        env.set_state(capture_entry_metrics=capture, **fields)
        ec.set_state(ora, capture_entry_metrics=capture, **fields)
        rows = ~run.tainted if run.tainted.any() else None       # (f32: an env that met a tie in the five steps may hold other counters)
        h = ec.compare_state(env, ora, real, stats, rows=rows, ctx=ctx)
        ec.compare_obs(env.current_observation().cpu().numpy(), ec.observe(ora), real, stats, rows=rows, ctx=ctx, name="current_observation")
        return h

    def fields_of(v, keys=ec.STATE_KEYS):
        return {k: v[ec.OPTION_OF_STATE[k]] for k in keys}

    counters = {k: env.info()[k].cpu().numpy().copy() for k in ("step_count", "dwell_count", "near_goal_entry_count", "near_goal_drift_count", "flags")}
    assert np.count_nonzero(counters["step_count"]) > N // 2       # (an env that just succeeded has been reset by the step)
    entry0 = env.info()["entry_metrics"].cpu().numpy().copy()
    h = place("all five, capture", True, **fields_of(draws[0]))
    for k, c in counters.items():      # a running episode keeps its counters
        assert np.array_equal(h[k], c), k
    assert not np.array_equal(h["entry_metrics"], entry0.T)
    assert np.array_equal(h["goal_pose6"], draws[0]["goal_pose6"] if real == "f64" else draws[0]["goal_pose6"].astype(np.float32).astype(np.float64))
    assert np.array_equal(h["q"], draws[0]["initial_q"] if real == "f64" else _two_float(draws[0]["initial_q"]))     # placed as given: no clipping
    for capture in (False, True):
        v = draws[2 if capture else 1]
        for k in ec.STATE_KEYS:
            before = h
            h = place(f"{k} alone, capture={capture}", capture, **fields_of(v, (k,)))
            if not capture:
                assert np.array_equal(h["entry_metrics"], before["entry_metrics"]), k
            for other in ec.STATE_KEYS:
                if other != k:
                    assert np.array_equal(h[other], before[other]), (k, other)
            if k != "q":
                assert np.array_equal(h["ee_pose6"], before["ee_pose6"]), k
    h = place("all five, no capture", False, **fields_of(draws[0]))
    for k, c in counters.items():
        assert np.array_equal(h[k], c), k
    run.run(20, ctx="from the placed state")
    stats.report(f"test_set_state_get_state_observe[{real}-{stride}]")
    env.close()


# ============================================================================== snapshot / restore
@pytest.mark.parametrize("real", ["f64", "f32"])
@pytest.mark.parametrize("name", [APPROACH, SHORT_DOCK])
def test_snapshot_restore_replays_bit_equal(name, real):
    """30 steps, snapshot, 40 recorded steps, restore, the same 40 steps again: every word of the state right after the restore and every
    recorded tensor is bit-equal; the oracle runs alongside (f64: every step compared; f32: its exact part).  The dock config is the one
    whose resets draw 32-bit variates (the hand-off index), so the buffered half-word of the PCG64 stream moves between snapshot and end;
    approach_default never touches it."""
    cfg, env, ora = _pair(name, real)
    stats = ec.Stats()
    run = ec.Lockstep(env, ora, cfg, real, stats)
    run.start()
    run.run(30)
    env.snapshot()
    snap, arng_state, tainted = ec.snapshot(ora), run.arng.bit_generator.state, run.tainted.copy()
    at_snapshot = ec.handle_arrays(env)
    first = [run.step(ctx="recording") for _ in range(40)]
    end = ec.handle_arrays(env)
    assert sum(int(np.count_nonzero(r["done"] & 3)) for r in first) >= N      # the recorded steps go through auto-resets
    assert not np.array_equal(end["rng"], at_snapshot["rng"])
    assert name != SHORT_DOCK or np.count_nonzero(np.any(end["rng"][:, 4:] != at_snapshot["rng"][:, 4:], axis=1)) > N // 2
    env.restore()
    ec.restore(ora, snap)
    run.arng.bit_generator.state, run.tainted = arng_state, tainted
    ec.assert_same_words(at_snapshot, ec.handle_arrays(env), ctx="right after the restore")
    again = [run.step(ctx="replay") for _ in range(40)]
    for t, (r1, r2) in enumerate(zip(first, again)):
        for k in ("obs", "reward", "done_handle"):
            assert torch.equal(r1[k], r2[k]), (t, k)
    ec.assert_same_words(end, ec.handle_arrays(env), ctx="after the replay")
    stats.report(f"test_snapshot_restore_replays_bit_equal[{name}-{real}]")
    env.close()


@pytest.mark.parametrize("real", ["f64", "f32"])
def test_snapshot_overwrite_and_restore_without_snapshot(real):
    cfg, env, ora = _pair(SHORT_DOCK, real)
    env.reset()
    before = ec.handle_arrays(env)
    with pytest.raises(ValueError):
        env.restore()                      # KP1_ERR_INVALID: there is no snapshot yet
    ec.assert_same_words(before, ec.handle_arrays(env), ctx="after the refused restore")
    gen = np.random.default_rng(4)

    def steps(k):
        for _ in range(k):
            env.step(_actions(env, gen.uniform(-1, 1, size=(N, 7))))

    env.snapshot()
    steps(7)
    env.snapshot()                         # overwrites the first
    second = ec.handle_arrays(env)
    steps(25)
    moved = ec.handle_arrays(env)["rng"]
    assert np.any(moved[:, :4] != second["rng"][:, :4]) and np.any(moved[:, 4:] != second["rng"][:, 4:])     # both halves of the stream state moved
    env.restore()
    ec.assert_same_words(second, ec.handle_arrays(env), ctx="restore returns the second snapshot")
    assert not np.array_equal(second["q"], before["q"])
    env.restore()                          # a snapshot can be restored more than once
    ec.assert_same_words(second, ec.handle_arrays(env), ctx="second restore")
    env.close()


# ============================================================================== mid-run changes
def _run_until_all_reset(run: ec.Lockstep, limit: int, each_step=None, ctx: str = "") -> None:
    run.resets[:] = 0
    k = 0
    while run.resets.min() == 0:
        assert k < limit, f"{ctx}: not every env reset within {limit} steps"
        rec = run.step(ctx=ctx)
        if each_step is not None:
            each_step(rec)
        k += 1


@pytest.mark.parametrize("real", ["f64", "f32"])
def test_midrun_stage_change(real):
    """set_curriculum_stage up, then down, in the middle of a run: running episodes keep their stage_index, every reset after the call draws
    from the new stage (approach_default's sampler draws the current stage only)"""
    cfg, env, ora = _pair(APPROACH, real, stage=1)
    stats = ec.Stats()
    limit = 2 * int(cfg.c.termination.max_episode_steps) + 2
    run = ec.Lockstep(env, ora, cfg, real, stats)
    run.start()
    run.run(25)
    assert np.all(env.info()["stage_index"].cpu().numpy()[~run.tainted] == 1)
    for old, new in ((1, 4), (4, 2)):
        env.set_curriculum_stage(new)
        ora.set_stage(new)
        assert env.get_curriculum_stage() == new
        assert np.all(env.info()["stage_index"].cpu().numpy()[~run.tainted] == old)            # the call itself moves no episode

        def check(rec, old=old, new=new):
            ok = ~run.tainted
            running = (run.resets == 0) & ok
            assert np.all(rec["stage_index"][running] == old) and np.all(rec["stage_index"][(run.resets > 0) & ok] == new)

        _run_until_all_reset(run, limit, check, ctx=f"stage {old} -> {new}")
        assert np.all(env.info()["stage_index"].cpu().numpy()[~run.tainted] == new)
    stats.report(f"test_midrun_stage_change[{real}]")
    env.close()


@pytest.mark.parametrize("tracker", [False, True], ids=["plain", "tracker"])
@pytest.mark.parametrize("real", ["f64", "f32"])
def test_midrun_config_change(real, tracker):
    """apply_dock_training_stage in the middle of a run.  Plain handle: the step that follows clips running episodes' actions to the new
    limit, later resets use the new dock_reset block.  With a dock curriculum tracker bound, the upload ends in the tracker's stage being
    applied again: what a stage can override goes back to the stage's value, the rest of the payload arrives."""
    cfg, env, ora = _pair(SHORT_DOCK, real)
    stats = ec.Stats()
    limit = 2 * int(cfg.c.termination.max_episode_steps) + 2
    cur = None
    if tracker:
        cur = ft.DockReverseCurriculum(stages=[{"name": "s0", "dock_residual_action_limit": 0.6, "init_q_noise": [0.03] * 7, "handoff_state_probability": 0.4},
                                               {"name": "s1", "dock_residual_action_limit": 0.2}], window_episodes=8)
        record = cur.resolved_stages(cfg)[0]
        cur.attach(env)                          # stage 0 goes into the device config before the first reset
        ec.apply_dock_stage(ora, record)
    run = ec.Lockstep(env, ora, cfg, real, stats)
    run.start()
    run.run(25)
    scale = 0.5 * float(cfg.c.env.dock_action_delta_scale or cfg.c.env.action_delta_scale)
    payload = {"dock_action_delta_scale": scale, "dock_residual_action_limit": 0.3, "dock_dynamic_residual_action_limit_near": 0.3,
               "dock_dynamic_residual_action_limit_far": 0.3,
               "dock_reset": {"init_q_noise": [0.01] * 7, "goal_noise": [0.02] * 7, "handoff_state_probability": 0.0, "close_bucket_probability": 0.0}}
    env.apply_dock_training_stage(payload)       # rewrites cfg.c (the env's config object) and uploads it
    assert cfg.c.env.dock_action_delta_scale == scale and list(cfg.c.dock_reset.goal_noise[:]) == [0.02] * 7
    ec.update_config(ora, cfg)
    if tracker:
        ec.apply_dock_stage(ora, record)
        assert ora.envs[0].cfg.env.dock_residual_action_limit == 0.6 and ora.envs[0].cfg.dock_reset.handoff_state_probability == 0.4
    goal_centre = np.array(cfg.c.dock_reset.goal_q[:])
    lo, hi = np.array(cfg.c.joints.lower[:]), np.array(cfg.c.joints.upper[:])

    seen = {"running": 0, "fresh": 0}

    def check(rec):
        if tracker:
            return
        ok = ~run.tainted
        running = (rec["step_count"] > 0) & ok
        pa = env.info()["prev_action"].double().cpu().numpy().T
        assert not running.any() or np.abs(pa[running]).max() <= 0.3 + 1e-6      # the new action limit holds for episodes already running
        seen["running"] += int(running.sum())
        seen["fresh"] += int(((rec["step_count"] == 0) & ok).sum())
        fresh = (rec["step_count"] == 0) & ok
        st = env.get_state()
        assert np.all(np.abs(st["goal_q"][fresh] - np.clip(goal_centre, lo, hi)) <= 0.02 + 1e-6)     # new goal_noise, no hand-off state
        assert np.all(np.abs(st["q"][fresh] - st["goal_q"][fresh]) <= 0.01 + 1e-6)                   # new init_q_noise, no close bucket

    _run_until_all_reset(run, limit, check, ctx="after the config change")
    assert tracker or (seen["running"] > N // 2 and seen["fresh"] >= N // 2), seen
    stats.report(f"test_midrun_config_change[{real}-{'tracker' if tracker else 'plain'}]")
    if cur is not None:
        cur.close()
    env.close()


@pytest.mark.parametrize("real", ["f64", "f32"])
def test_midrun_handoff_buffer_change(real):
    """set_handoff_states in the middle of a run: a shorter buffer, then an empty one (the sampler falls back to the sampled dock reset and
    draws no hand-off variate at all, as the oracle does); drawn indices and RNG words exact"""
    cfg, env, ora = _pair(SHORT_DOCK, real)
    stats = ec.Stats()
    limit = 2 * int(cfg.c.termination.max_episode_steps) + 2
    original = list(cfg.handoff_states)
    cast = (lambda x: x) if real == "f64" else _two_float
    old_pool = cast(np.array([s["initial_q"] for s in original]))
    run = ec.Lockstep(env, ora, cfg, real, stats)
    run.start()
    run.run(25)
    shorter = original[40:5:-3]
    assert 0 < len(shorter) != len(original)
    new_pool = cast(np.array([s["initial_q"] for s in shorter]))
    drawn = {"new": 0, "old": 0}

    def member(pool, q):
        return np.array([bool(np.any(np.all(pool == row, axis=1))) for row in q], bool)

    def check(rec):
        fresh = (rec["step_count"] == 0) & ~run.tainted
        q = env.get_state()["q"][fresh]
        in_new, in_old = member(new_pool, q), member(old_pool, q)
        drawn["new"] += int(in_new.sum())
        drawn["old"] += int((in_old & ~in_new).sum())

    env.set_handoff_states(shorter)
    ec.set_handoff(ora, shorter)
    _run_until_all_reset(run, limit, check, ctx="shorter buffer")
    assert drawn["new"] > N // 4 and drawn["old"] == 0, drawn                  # handoff_state_probability is 0.5
    drawn.update(new=0, old=0)
    env.set_handoff_states([])
    ec.set_handoff(ora, [])
    new_pool = old_pool
    _run_until_all_reset(run, limit, check, ctx="empty buffer")
    assert drawn["new"] == 0 and drawn["old"] == 0, drawn
    stats.report(f"test_midrun_handoff_buffer_change[{real}]")
    env.close()


@pytest.mark.parametrize("real", ["f64", "f32"])
def test_midrun_mode_change(real):
    """set_policy_mode to the other mode mid-episode, stepped without auto-reset: reward, termination and the observation's mode flag follow
    the oracle in that mode; a reset without options returns to the config's mode on both sides"""
    cfg, env, ora = _pair(APPROACH, real)
    stats = ec.Stats()
    run = ec.Lockstep(env, ora, cfg, real, stats)
    run.start()
    run.run(25)
    _assert_mode(env.obs, "approach")
    env.set_policy_mode("dock")
    ec.set_mode(ora, "dock")
    for _ in range(12):
        rec = run.step(auto_reset=False, ctx="dock mode")
        _assert_mode(rec["obs"], "dock")
        _assert_mode(ora.obs, "dock")
    _assert_mode(env.current_observation(), "dock")
    obs = env.reset().cpu().numpy()
    obs_o = ec.reset(ora)
    _assert_mode(obs, "approach")
    ec.compare_state(env, ora, real, stats, ctx="reset after the mode change")
    ec.compare_obs(obs, obs_o, real, stats, ctx="reset after the mode change", name="reset observation")
    run.tainted[:] = False                       # every env starts a new episode from exact words
    for _ in range(5):
        _assert_mode(run.step(ctx="back in approach mode")["obs"], "approach")
    stats.report(f"test_midrun_mode_change[{real}]")
    env.close()


def test_policy_mode_override_is_handle_wide():
    """What the handle does with a ``policy_mode`` override that differs from the config's mode (module docstring): the auto-reset inside
    kp1_step resets in the overriding mode -- it equals ``reset(options={"policy_mode": mode})`` of the finished env, not the reference's
    reset without options -- and a masked override switches the envs outside the mask as well.  ``reset()`` without options ends it."""
    cfg, env, ora = _pair(APPROACH, "f64")
    stats = ec.Stats()
    opts = {"policy_mode": "dock"}
    ec.compare_obs(env.reset(options=opts).cpu().numpy(), ec.reset(ora, opts), "f64", stats, ctx="override reset")
    arng = np.random.default_rng(6)
    resets = np.zeros(N, np.int64)
    t = 0
    while resets.min() < 2:
        assert t < 5 * int(cfg.c.termination.max_episode_steps)
        a = ec.draw_actions(arng, ora, cfg)
        og, rg, dg = env.step(_actions(env, a))
        out = ora.step_out(a)
        done = (out["terminated"] | (out["truncated"] << 1) | (out["success"] << 2) | (out["invalid"] << 3)).astype(np.uint8)
        for i in np.nonzero(done & 3)[0]:
            ora.reset_env(int(i), opts)          # the handle-wide rule; the reference would call reset_env(i) here
        resets += (done & 3) != 0
        assert np.array_equal(dg.cpu().numpy(), done), t
        stats.within("f64 step reward", np.abs(rg.cpu().numpy() - out["reward"]), ec.F64_REWARD_TOL, f"step {t}")
        stats.within("f64 step observation", np.abs(og.cpu().numpy() - ora.obs), ec.F64_OBS_TOL, f"step {t}")
        assert np.array_equal(env.rng_state(), ora.rng_words()), t
        _assert_mode(og, "dock", ctx=f"step {t}")
        t += 1
    h = ec.compare_state(env, ora, "f64", stats, ctx="after the auto-resets in dock mode", norms=False)
    if np.any(h["step_count"] > 0):        # (a dock reset starts next to its goal: most envs succeed, and are reset, every step)
        ec.compare_state(env, ora, "f64", stats, rows=h["step_count"] > 0, ctx="after the auto-resets in dock mode, running episodes", h=h)
    obs = env.reset().cpu().numpy()
    _assert_mode(obs, "approach")
    ec.compare_obs(obs, ec.reset(ora), "f64", stats, ctx="reset without options")
    # a masked override: the envs outside the mask keep their state words, but the handle's one mode is theirs too
    mask = ec.reset_mask()
    env.reset(options=opts, mask=torch.tensor(mask, device="cuda"))
    _assert_mode(env.current_observation(), "dock")
    ec.reset(ora, opts, mask)
    ec.set_mode(ora, "dock")
    ec.compare_state(env, ora, "f64", stats, ctx="masked override")
    ec.compare_obs(env.current_observation().cpu().numpy(), ec.observe(ora), "f64", stats, ctx="masked override", name="current_observation")
    stats.report("test_policy_mode_override_is_handle_wide")
    env.close()


# ============================================================================== populations
def _population(seeds=(31, 977)):
    cfg = load_golden_config(APPROACH)
    n = N // len(seeds)
    pop = ArmKinematicPopulationVecEnv(cfg, list(seeds), n)
    singles = [ArmKinematicVecEnv(cfg, n, seed=s, real="f32") for s in seeds]
    for e in (pop, *singles):
        e.set_curriculum_stage(STAGE[APPROACH])
    return cfg, n, pop, singles


def _assert_population_equals_singles(pop, singles, ctx: str) -> None:
    hp = ec.handle_arrays(pop)
    hs = [ec.handle_arrays(e) for e in singles]
    for k in hp:
        assert np.array_equal(hp[k], np.concatenate([h[k] for h in hs])), f"{ctx}: {k}"


def _step_population(pop, singles, n, gen, steps: int, ctx: str) -> None:
    for t in range(steps):
        a = torch.tensor(gen.uniform(-1, 1, size=(pop.n_envs, 7)), dtype=torch.float32, device="cuda")
        obs, rew, done = pop.step(a)
        for k, e in enumerate(singles):
            o, r, d = e.step(a[k * n:(k + 1) * n].contiguous())
            assert torch.equal(obs[k * n:(k + 1) * n], o) and torch.equal(rew[k * n:(k + 1) * n], r) and torch.equal(done[k * n:(k + 1) * n], d), (ctx, t, k)


def test_population_snapshot_restore_equals_single_handles():
    cfg, n, pop, singles = _population()
    assert pop.n_envs == N
    gen = np.random.default_rng(8)
    assert torch.equal(pop.reset(), torch.cat([e.reset() for e in singles]))
    _step_population(pop, singles, n, gen, 12, "before the snapshot")
    for e in (pop, *singles):
        e.snapshot()
    at_snapshot = ec.handle_arrays(pop)
    _step_population(pop, singles, n, gen, 25, "after the snapshot")
    for e in (pop, *singles):
        e.restore()
    ec.assert_same_words(at_snapshot, ec.handle_arrays(pop), ctx="population restore")
    _assert_population_equals_singles(pop, singles, "after the restore")
    _step_population(pop, singles, n, gen, 25, "after the restore")
    _assert_population_equals_singles(pop, singles, "end")
    for e in (pop, *singles):
        e.close()


def test_population_masked_reset_options_equals_single_handles():
    cfg, n, pop, singles = _population()
    gen = np.random.default_rng(9)
    v = ec.draw_options(cfg)
    mask = ec.reset_mask()
    pop.reset()
    for e in singles:
        e.reset()
    _step_population(pop, singles, n, gen, 5, "before the resets")
    for keys in (ec.OPTION_KEYS, ("initial_q",), ("goal_pose6",), ("initial_dq", "initial_prev_action"), ("initial_q", "goal_q")):
        before = ec.handle_arrays(pop)
        opts = {k: v[k] for k in keys}
        obs = pop.reset(options=opts, mask=torch.tensor(mask, device="cuda")).clone()
        for k, e in enumerate(singles):
            rows = slice(k * n, (k + 1) * n)
            o = e.reset(options={key: val[rows] for key, val in opts.items()}, mask=torch.tensor(mask[rows], device="cuda"))
            sel = torch.tensor(mask[rows].astype(bool), device="cuda")
            assert torch.equal(obs[rows][sel], o[sel]), (keys, k)
        _assert_population_equals_singles(pop, singles, f"masked reset {keys}")
        ec.assert_same_words(before, ec.handle_arrays(pop), rows=~mask.astype(bool), ctx=f"masked reset {keys}: env outside the mask")
        _step_population(pop, singles, n, gen, 3, f"after masked reset {keys}")
    with pytest.raises(ValueError):
        pop.reset(options={"policy_mode": "dock"})
    for e in (pop, *singles):
        e.close()
