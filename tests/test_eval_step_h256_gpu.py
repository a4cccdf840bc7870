"""The one-launch evaluation step of 2x256 policies (kp1_eval_step on the evaluation form of the inference tile, mlp_tile_kernel<false, 2, 3 | 4>)
and the host paths that take it, on the GPU.

Shapes: E = 70 rows (three 32-row tiles, the last ragged) plus E = 1, 32, 33 for one mode; weights of differently seeded ActorCritic(256) with
the action head scaled up so that part of the mean actions leave [-1, 1] and the clamp is exercised.  Configs: workspace_expansion_bigtrain
(approach) and dock_workspace_handoff_noop_ft_12env_raw (dock).
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest
import torch

import eval_forms as F
import trained_regime as T
from conftest import load_golden_config
from eval_forms import DEV, NORM_RTOL, THR
from rl_brain_trainer_amd import evaluate as ev
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import ppo as P
from rl_brain_trainer_amd import workspace_coverage as wc
from rl_brain_trainer_amd.mlp import MlpKernels
from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

pytestmark = pytest.mark.gpu
E = 70
UNSUPPORTED = -4          # KP1_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def policies():
    """three differently seeded 2x256 InferencePolicy; their MlpKernels are the K = 1 handles of the one-launch runs"""
    return [P.InferencePolicy(F.state_dict(256, 21 + k), device=DEV, max_batch=128) for k in range(3)]


def _cfg(mode: str):
    return load_golden_config("workspace_expansion_bigtrain" if mode == "approach" else "dock_workspace_handoff_noop_ft_12env_raw")


@pytest.fixture(scope="module")
def suite():
    """70 explicit resets: 35 episodes each of two stages of workspace_expansion_bigtrain's curriculum-local suite"""
    return F.build_suite(_cfg("approach"), E // 2)


def _opts(suite, mode: str, n: int = E) -> dict:
    return {**{k: v[:n] for k, v in suite.items()}, "policy_mode": mode}


# ---------------------------------------------------------------------------------------------------------------- 1. step parity
def _step_parity(pol, suite, mode: str, stride: int, confirm: int, n: int, fp64_flat: torch.Tensor | None = None) -> None:
    """``fp64_flat``: the policy's parameters, for a check of the first step's deterministic action against an fp64 forward of the
    observations the env holds at that step, under the forward tolerances"""
    L = native.load()
    opts = _opts(suite, mode, n)
    active = F.forced_active_mask(n)
    env, ref_env = F.make_env(_cfg(mode), n, stride, opts), F.make_env(_cfg(mode), n, stride, opts)
    b, rb = ev.EpisodeBuffers(n, DEV, want_hand=True), ev.EpisodeBuffers(n, DEV, want_hand=True)
    thr = (C.c_double * 4)(*THR)
    for e_, b_ in ((env, b), (ref_env, rb)):
        native.check(L.kp1_eval_accumulate(e_._handle, C.byref(b_.struct), None, None, F.ptr(active), 0, thr, confirm, F.stream()))
    at_clamp = inside = 0
    for step in range(1, env.config.c.termination.max_episode_steps + 2):      # to the episode limit + 1
        native.check(L.kp1_eval_step(pol._mlp._h, env._handle, F.ptr(env.obs), F.ptr(env.reward), F.ptr(env.done), C.byref(b.struct), step, thr, confirm,
                                     F.stream()))
        action = pol.predict(ref_env.obs)
        if fp64_flat is not None and step == 1:
            T.assert_step_against_fp64(fp64_flat, 256, 56, ref_env.obs, None, {"clipped": action}, "step 1, deterministic action")
        at_clamp += int((action.abs() == 1.0).sum())
        inside += int((action.abs() < 1.0).sum())
        an = F.norm_in_index_order(action)
        ref_env.step(action, auto_reset=False)
        native.check(L.kp1_eval_accumulate(ref_env._handle, C.byref(rb.struct), F.ptr(an), F.ptr(ref_env.done), None, step, thr, confirm,
                                           F.stream()))
        assert torch.equal(env.obs, ref_env.obs), ("obs", step)
        assert torch.equal(env.done, ref_env.done), ("done", step)
        assert torch.equal(env.reward, ref_env.reward), ("reward", step)
        fi, ri = env.info(), ref_env.info()
        for k in ri:
            assert torch.equal(fi[k], ri[k]), (k, step)
        assert torch.equal(b.n_alive, rb.n_alive), ("n_alive", step)
    for name in F.NAMES:
        assert torch.equal(getattr(b, name), getattr(rb, name)), name
    if n == E:
        assert at_clamp > 0 and inside > 0                                  # the clamp was met, and not everywhere
    assert int(rb.n_alive) == 0 and int(rb.counters[0].max()) >= 2           # episodes ran, and to their end
    assert bool((rb.flags[0] == 0).all()) and torch.equal(rb.counters[0][active == 0], torch.zeros_like(rb.counters[0][active == 0]))
    if confirm == 0:
        assert torch.equal(rb.flags[3], active)                              # ready_streak >= 0 hands over at step 1
    env.close()
    ref_env.close()


@pytest.mark.parametrize("confirm", [0, 2])
@pytest.mark.parametrize("stride", [56, 64])
@pytest.mark.parametrize("mode", ["approach", "dock"])
def test_eval_step_h256_equals_the_launch_sequence(policies, suite, mode, stride, confirm):
    """kp1_eval_step on a 2x256 handle against InferencePolicy.predict + the norm written out term by term + env.step(auto_reset=False) +
    kp1_eval_accumulate on a second env handle: after EVERY step the observation buffer, the done bytes, the reward and every env.info()
    field, at the end every eval buffer, bit for bit."""
    _step_parity(policies[0], suite, mode, stride, confirm, E)


@pytest.mark.parametrize("n", [1, 32, 33])
def test_eval_step_h256_row_counts(policies, suite, n):
    """one row, exactly one tile, one tile and one row"""
    _step_parity(policies[0], suite, "approach", 56, 2, n)


def test_eval_step_h256_trained_scale(suite):
    """the T4 policy of tests/trained_regime.py (40 % of the second-layer units beyond |h| = 0.999) on one tile and one row: the same bit
    equality after every step, and the first step's action against fp64.  (The action reaches the env only through the one-launch step on
    one twin and through predict on the other, and the observations after the step are equal bit for bit.)"""
    trained = T.trained_policy(256, 56, "T4")
    pol = P.InferencePolicy(trained.state_dict(), device=DEV, max_batch=128)
    _step_parity(pol, suite, "approach", 56, 2, 33, fp64_flat=trained.flat)


# ---------------------------------------------------------------------------------------------------------------- 2. runner and evaluators
@pytest.mark.parametrize("mode,confirm", [("approach", 2), ("approach", None), ("dock", 2), ("dock", None)])
def test_run_episodes_fused_h256_equals_run_episodes(policies, suite, mode, confirm):
    pol = policies[1]
    ready = F.READY
    active = F.forced_active_mask(E).bool()
    assert ev._is_fused_width(pol._mlp) and ev.policy_mlp(pol.predict) is pol._mlp and ev.policy_mlp(pol) is pol._mlp
    out = []
    for fused in (True, False):
        env = ArmKinematicVecEnv(_cfg(mode), E, seed=3)
        env.set_obs_stride(64)
        if fused:
            out.append(ev.run_episodes_fused(env, pol._mlp, _opts(suite, mode), ready_cfg=ready, handoff_confirm_steps=confirm, active=active))
        else:
            out.append(ev.run_episodes(env, pol.predict, _opts(suite, mode), ready_cfg=ready, handoff_confirm_steps=confirm, active=active))
        env.close()
    (res, hand), (ref, ref_hand) = out
    F.assert_results_match(res, ref, "final")
    assert (hand is None) == (ref_hand is None) == (confirm is None)
    if hand is not None:
        F.assert_results_match(hand, ref_hand, "handoff")
    assert int(ref["step_count"].max()) >= 2


def _count_calls(monkeypatch):
    calls = {"fused": 0, "launches": 0}
    fused, plain = ev.run_episodes_fused, ev.run_episodes

    def fused_(*a, **k):
        calls["fused"] += 1
        return fused(*a, **k)

    def plain_(*a, **k):
        calls["launches"] += 1
        return plain(*a, **k)

    monkeypatch.setattr(ev, "run_episodes_fused", fused_)
    monkeypatch.setattr(ev, "run_episodes", plain_)
    return calls


def test_evaluate_workspace_expansion_one_launch_equals_multi_launch(tmp_path, monkeypatch, policies):
    """evaluate_workspace_expansion(one_launch=None) -- both phases through the one-launch step -- against one_launch=False: payloads equal
    (action-magnitude floats to the tolerance), the JSON files parse to the payloads.  handoff_confirm_steps = 0 hands every episode over at
    step 1, so the 2x256 Finisher phase runs."""
    calls = _count_calls(monkeypatch)
    acfg, fcfg = _cfg("approach"), _cfg("dock")
    kw = dict(approach_policy=policies[1].predict, finisher_policy=policies[2], approach_cfg=acfg, finisher_cfg=fcfg, episodes=4, seed=700001,
              stage_indices=[0, 3], handoff_confirm_steps=0, gate_config={"score_stage_index": 3})
    got = ev.evaluate_workspace_expansion(artifact_root=tmp_path / "one", **kw)
    assert calls == {"fused": 2, "launches": 0}
    ref = ev.evaluate_workspace_expansion(artifact_root=tmp_path / "multi", one_launch=False, **kw)
    assert calls == {"fused": 2, "launches": 2}
    F.assert_payload_match(got, ref)
    assert len(got["target_rows"]) == 8
    for root, payload in ((tmp_path / "one", got), (tmp_path / "multi", ref)):
        assert json.loads((root / "workspace_eval_summary.json").read_text()) == json.loads(json.dumps(payload))
        assert json.loads((root / "stage_metrics.json").read_text()) == json.loads(json.dumps(payload["stage_metrics"]))
        assert json.loads((root / "best_model_selection_summary.json").read_text()) == json.loads(json.dumps(payload["best_model_selection"]))


def test_run_pairs_columns_one_launch_equals_multi_launch(monkeypatch, policies):
    """wc._run_pairs_columns on 96 pairs from small maps, Approach and Finisher both 2x256: the columns of the two forms"""
    calls = _count_calls(monkeypatch)
    cfg = load_golden_config("workspace_full_coverage_randomstart_overnight")
    fk = wc._device_fk(0)
    targets, _ = wc.generate_workspace_target_map(cfg, seed=940002, stage_samples_per_stage=8, random_samples=64, fk=fk)
    starts, _ = wc.generate_workspace_start_state_map(cfg, seed=940003, stage_samples_per_stage=4, random_samples=64, fk=fk)
    pairs, _ = wc.build_pair_sampler_summary(starts=starts, targets=targets, seed=940004, pair_count=96)
    common = dict(pairs=pairs, starts_by_id={r["start_id"]: r for r in starts}, targets_by_id={r["target_id"]: r for r in targets},
                  approach_policy=policies[1].predict, approach_cfg=cfg, finisher_policy=policies[2].predict, finisher_cfg=_cfg("dock"),
                  handoff_confirm_steps=0, device=0, obs_stride=64, seed=760001, first_env_id=96)
    got = wc._run_pairs_columns(**common)
    assert calls == {"fused": 2, "launches": 0}
    ref = wc._run_pairs_columns(one_launch=False, **common)
    assert calls == {"fused": 2, "launches": 2}
    assert got.shape == ref.shape == (96, len(wc._COLS))
    for k, name in enumerate(wc._COLS):
        if name.endswith("final_action_magnitude"):
            assert torch.allclose(got[:, k], ref[:, k], rtol=NORM_RTOL, atol=0.0), name
        else:
            assert torch.equal(got[:, k], ref[:, k]), name
    assert float(got[:, wc._COLS.index("approach_steps")].min()) >= 1


# ---------------------------------------------------------------------------------------------------------------- 3. training handle
_TRAIN_EVAL_KW = dict(finisher_policy=None, finisher_cfg=None, episodes=4, seed=700001, stage_indices=[0, 3], handoff_confirm_steps=2)


def test_training_handle_evaluates_like_a_fresh_inference_policy(monkeypatch):
    """after one iteration with graphs on, ppo.predict resolves to the TRAINING handle; its one-launch evaluation equals the one through a
    fresh InferencePolicy built from the state dict (same weights packed anew): every float, the action magnitudes included -- both run the
    same kernel"""
    calls = _count_calls(monkeypatch)
    ppo, env = F.trained_ppo(_cfg("approach"))
    assert ev.policy_mlp(ppo.predict) is ppo._mlp and ev._is_fused_width(ppo._mlp)
    got = ev.evaluate_workspace_expansion(approach_policy=ppo.predict, approach_cfg=_cfg("approach"), obs_stride=ppo.obs_w, **_TRAIN_EVAL_KW)
    fresh = P.InferencePolicy({k: v.clone() for k, v in ppo.policy.state_dict().items()}, device=DEV)
    ref = ev.evaluate_workspace_expansion(approach_policy=fresh.predict, approach_cfg=_cfg("approach"), obs_stride=ppo.obs_w, **_TRAIN_EVAL_KW)
    assert calls == {"fused": 2, "launches": 0}
    assert got == ref
    multi = ev.evaluate_workspace_expansion(approach_policy=ppo.predict, approach_cfg=_cfg("approach"), obs_stride=ppo.obs_w, one_launch=False, **_TRAIN_EVAL_KW)
    F.assert_payload_match(got, multi)
    env.close()


def test_evaluation_on_the_training_handle_leaves_training_untouched():
    """parameters, Adam moments, env info, RNG state and the rollout observation buffer after [iteration, evaluation, iteration] == after
    [iteration, iteration]: the step reads the training handle's packed weights and writes nothing of the handle's"""
    out = []
    for evaluate in (True, False):
        ppo, env = F.trained_ppo(_cfg("approach"))
        if evaluate:
            ev.evaluate_workspace_expansion(approach_policy=ppo.predict, approach_cfg=_cfg("approach"), obs_stride=ppo.obs_w, **_TRAIN_EVAL_KW)
        ppo.learn(256 * 8)
        torch.cuda.synchronize()
        out.append((ppo.policy.flat.clone(), ppo.adam_m.clone(), ppo.adam_v.clone(), ppo.obs_buf.clone(), ppo.gens[0].get_state().clone(),
                    {k: v.clone() for k, v in env.info().items()}, env.rng_state()))
        env.close()
    a, b = out
    assert all(torch.equal(x, y) for x, y in zip(a[:5], b[:5]))
    assert all(torch.equal(a[5][k], b[5][k]) for k in a[5]) and np.array_equal(a[6], b[6])


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def _refused(mlp: MlpKernels, env: ArmKinematicVecEnv, status: int, text: str) -> None:
    """kp1_eval_step refuses with `status` and `text` in kp1_last_error, and launches nothing: no buffer, observation or env field changes"""
    L = native.load()
    b = ev.EpisodeBuffers(env.n_envs, DEV, want_hand=True)
    for name in F.NAMES:
        getattr(b, name).fill_(7)
    before = (env.obs.clone(), {k: v.clone() for k, v in env.info().items()})
    L.kp1_last_error.restype = C.c_char_p
    rc = L.kp1_eval_step(mlp._h, env._handle, F.ptr(env.obs), F.ptr(env.reward), F.ptr(env.done), C.byref(b.struct), 1, None, 0, F.stream())
    assert rc == status, (rc, L.kp1_last_error())
    assert text in L.kp1_last_error().decode(), L.kp1_last_error()
    torch.cuda.synchronize()
    for name in F.NAMES:
        assert bool((getattr(b, name) == 7).all()), name
    assert torch.equal(env.obs, before[0]) and all(torch.equal(v, before[1][k]) for k, v in env.info().items())


def test_refusals(policies, suite):
    opts = _opts(suite, "approach", 8)
    env = F.make_env(_cfg("approach"), 8, 56, opts)
    off = MlpKernels(256, DEV, max_batch=64)
    off.pack(policies[0].policy.flat)
    assert ev._is_fused_width(off)
    off.set_fused(False)
    assert not ev._is_fused_width(off)
    _refused(off, env, UNSUPPORTED, "needs the tile kernels")
    off.close()
    wide = MlpKernels(256, DEV, max_batch=64, obs_dim=80)
    assert not ev._is_fused_width(wide)
    _refused(wide, env, UNSUPPORTED, "56-float observation")
    wide.close()
    env.close()
    env64 = F.make_env(_cfg("approach"), 8, 56, opts, real="f64")
    _refused(policies[0]._mlp, env64, UNSUPPORTED, "fp32 handle")
    env64.close()
    comps = F.make_env(_cfg("approach"), 8, 56, opts, reward_components=True)
    _refused(policies[0]._mlp, comps, UNSUPPORTED, "reward components")
    comps.close()


def test_one_launch_true_refuses_a_policy_without_a_handle(policies):
    def servo(obs):
        return torch.tanh(obs[:, :7])

    kw = dict(finisher_policy=None, approach_cfg=_cfg("approach"), finisher_cfg=None, episodes=2, stage_indices=[0])
    with pytest.raises(ValueError, match="one_launch=True"):
        ev.evaluate_workspace_expansion(approach_policy=servo, one_launch=True, **kw)
    with pytest.raises(ValueError, match="one_launch=True"):
        ev.evaluate_workspace_expansion(approach_policy=lambda o: policies[0].predict(o), one_launch=True, **kw)
    ev.evaluate_workspace_expansion(approach_policy=policies[0].predict, one_launch=True, **kw)       # covered: runs


def test_evaluate_dock_one_launch_equals_multi_launch(monkeypatch):
    """train_dock.evaluate_dock with its resets drawn by the env (reset options None) through the one-launch step against the launch
    sequence: the same env seed draws the same resets, and the summary (which holds no action-norm float) is equal key by key"""
    from rl_brain_trainer_amd import train_dock

    calls = _count_calls(monkeypatch)
    env = ArmKinematicVecEnv(_cfg("dock"), 64, seed=11)
    ppo = P.PPO(env, P.PPOConfig(n_steps=4, batch_size=256, n_epochs=1, hidden=256, seed=11), use_graphs=False)
    ppo.policy.views["action_net.weight"].mul_(250.0)
    ppo._mlp.pack(ppo.policy.flat)
    kw = dict(episodes=70, seed=10_011, device=0)
    got = train_dock.evaluate_dock(ppo, _cfg("dock"), **kw)
    assert calls == {"fused": 1, "launches": 0}
    ref = train_dock.evaluate_dock(ppo, _cfg("dock"), one_launch=False, **kw)
    assert calls == {"fused": 1, "launches": 1}
    assert got == ref and got["episodes"] == 70 and got["mean_episode_length"] >= 2.0
    env.close()
