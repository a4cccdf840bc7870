"""Whole-rollout kernel (kp1_rollout_run) on the GPU: all env steps of a span in one launch, the critic in a second, and
optionally the curriculum tracker inside the first.  The reference is always a twin env (and twin tracker) created with the same seeds and
driven step by step with forward_env_step + observe; every comparison is torch.equal / np.array_equal / bytes equality."""
from __future__ import annotations

import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import trained_regime as TR
from conftest import GOLDEN, load_golden_config
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KP1_ERR_INVALID, KP1_ERR_UNSUPPORTED = -1, -4     # include/kp1.h
DOCK_CFG = "dock_workspace_handoff_noop_ft_12env_raw"
EPISODE_STEPS = 10        # max_episode_steps of the test config: 24 steps hold two truncations of every env
T_SPAN = 24
OUTPUTS = ("obs", "action", "log_prob", "value", "reward", "done", "terminal_obs")
TRAINER_BUFFERS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf", "term_obs_buf")


def _approach_cfg(episode_steps: int = EPISODE_STEPS):
    cfg = kcfg.to_env_config(kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"))
    assert cfg.c.curriculum_enabled and cfg.n_stages >= 8
    cfg.c.termination.max_episode_steps = episode_steps
    return cfg


def _bytes(obj) -> bytes:
    return bytes(C.string_at(C.addressof(obj), C.sizeof(obj)))


def _random_policy(hidden: int, K: int, seed: int, regime: str | None = None) -> torch.Tensor:
    """``regime``: the trained-scale policies of tests/trained_regime.py in place of the drawn ones"""
    from rl_brain_trainer_amd.ppo import ActorCritic

    if regime is not None:
        return torch.stack([TR.trained_policy(hidden, 56, regime, seed=seed + k).flat for k in range(K)]).to(DEV).contiguous()
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    rows = []
    for k in range(K):
        pol = ActorCritic(hidden, DEV, seed=seed + k)
        pol.views["action_net.weight"].mul_(25.0)
        for name, v in pol.views.items():
            if name.endswith("bias"):
                v.copy_((torch.rand(v.shape, generator=g) * 0.2 - 0.1).to(DEV))
        pol.views["log_std"].copy_((-1.3 + 1.1 * torch.rand(7, generator=g)).to(DEV))
        rows.append(pol.flat.clone())
    return torch.stack(rows).contiguous()


def _mlp(hidden: int, K: int, seed: int, max_batch: int = 128, regime: str | None = None):
    from rl_brain_trainer_amd.mlp import MlpKernels

    mlp = MlpKernels(hidden, DEV, max_batch=max_batch, replicas=K)
    flat = _random_policy(hidden, K, seed, regime)
    mlp.pack(flat if K > 1 else flat[0].contiguous())
    return mlp


def _make(K: int, n: int, pitch: int, tracker: dict | None, episode_steps: int = EPISODE_STEPS):
    """an env of K replicas x n envs (K = 1: the plain env on stage 5) and its attached tracker (``tracker``: PointCurriculum settings plus
    ``initial``, or None)"""
    from rl_brain_trainer_amd.curriculum import PointCurriculum, PointCurriculumPopulation
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    cfg = _approach_cfg(episode_steps)
    cur = None
    if K == 1:
        env = ArmKinematicVecEnv(cfg, n, seed=31)
        env.set_curriculum_stage(5)
        if tracker is not None:
            kw = {k: v for k, v in tracker.items() if k not in ("initial", "preseed")}
            cur = PointCurriculum(**kw, initial_stage_index=tracker["initial"])
    else:
        env = ArmKinematicPopulationVecEnv(cfg, list(range(7, 7 + K)), n)
        if tracker is not None:
            kw = {k: v for k, v in tracker.items() if k not in ("initial", "preseed")}
            cur = PointCurriculumPopulation(**kw, initial_stage_indices=tracker["initial"])
    if cur is not None:
        cur.attach(env)
        _preseed(cur, K, n, int(tracker.get("preseed", 0)))
    env.set_obs_stride(pitch)
    return env, cur


def _preseed(cur, K: int, n: int, episodes: int) -> None:
    """feed the tracker(s) `episodes` successful episodes through the per-step observe kernel before the span: a window that holds successes,
    a head that has wrapped and a non-zero window sum, the same on every twin"""
    left = episodes
    while left > 0:
        d = torch.zeros((K, n), dtype=torch.uint8, device=DEV)
        d[:, :min(left, n)] = native.DONE_TERMINATED | native.DONE_SUCCESS
        cur.observe(d.view(-1), n)
        left -= n


def _buffers(T: int, rows: int, pitch: int) -> dict:
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=DEV)   # noqa: E731
    return {"obs": z(T + 1, rows, pitch), "action": z(T, rows, 7), "log_prob": z(T, rows), "value": z(T, rows), "reward": z(T, rows),
            "done": z(T, rows, dt=torch.uint8), "terminal_obs": z(T, rows, pitch)}


def _noise(T: int, rows: int, seed: int) -> torch.Tensor:
    return torch.randn((T, rows, 7), generator=torch.Generator(device=DEV).manual_seed(99 + seed), device=DEV)


def _read_trackers(cur, K: int) -> list:
    if cur is None:
        return []
    return [cur.read()] if K == 1 else [cur.read(k) for k in range(K)]


def _final_state(env, cur, K: int) -> dict:
    torch.cuda.synchronize()
    return {"info": {k: v.clone() for k, v in env.info().items()}, "rng": np.array(env.rng_state()).copy(),
            "trackers": [_bytes(s) for s in _read_trackers(cur, K)]}


@functools.lru_cache(maxsize=None)
def _reference(hidden: int, pitch: int, n: int, K: int, T: int, tracker_key: tuple | None, episode_steps: int = EPISODE_STEPS, regime: str | None = None):
    """the per-step path on a twin: forward_env_step + observe for T steps.  Returns (buffers, final state, per-step tracker records).  Computed
    once per case and shared; nothing modifies it."""
    tracker = dict(tracker_key) if tracker_key is not None else None
    if tracker is not None and isinstance(tracker["initial"], tuple):
        tracker["initial"] = list(tracker["initial"])
    env, cur = _make(K, n, pitch, tracker, episode_steps)
    mlp = _mlp(hidden, K, seed=hidden + n, regime=regime)
    rows = K * n
    b = _buffers(T, rows, pitch)
    noise = _noise(T, rows, n)
    b["obs"][0].copy_(env.reset())
    steps = []          # per step: [(n_events, stage_episode_count, stage_index) of every tracker]
    for t in range(T):
        mlp.forward_env_step(env, b["obs"][t], noise=noise[t], value=b["value"][t], action=b["action"][t], log_prob=b["log_prob"][t],
                             next_obs=b["obs"][t + 1], reward=b["reward"][t], done=b["done"][t], terminal_obs=b["terminal_obs"][t])
        if cur is not None:
            cur.observe(b["done"][t], n)
            if T <= 64:
                steps.append([(int(s.n_events), int(s.stage_episode_count), int(s.stage_index)) for s in _read_trackers(cur, K)])
    final = _final_state(env, cur, K)
    mlp.close()
    if cur is not None:
        cur.close()
    env.close()
    return b, final, steps


def _run(hidden: int, pitch: int, n: int, K: int, T: int, tracker: dict | None, *, spans=None, skip: tuple = (), episode_steps: int = EPISODE_STEPS,
         regime: str | None = None):
    """the code under test on a fresh twin: rollout_run over ``spans`` (default: one span [0, T)); outputs named in ``skip`` are passed as None"""
    env, cur = _make(K, n, pitch, tracker, episode_steps)
    mlp = _mlp(hidden, K, seed=hidden + n, regime=regime)
    rows = K * n
    b = _buffers(T, rows, pitch)
    noise = _noise(T, rows, n)
    b["obs"][0].copy_(env.reset())
    for first, count in (spans or [(0, T)]):
        mlp.rollout_run(env, b["obs"], noise=noise, value=None if "value" in skip else b["value"], action=b["action"],
                        log_prob=None if "log_prob" in skip else b["log_prob"], reward=b["reward"], done=b["done"],
                        terminal_obs=None if "terminal_obs" in skip else b["terminal_obs"], first_step=first, n_steps=count, trackers=cur,
                        steps_per_call=n)
    final = _final_state(env, cur, K)
    mlp.close()
    if cur is not None:
        cur.close()
    env.close()
    return b, final


def _assert_equal(got, ref, skip: tuple = ()) -> None:
    (gb, gf), (rb, rf) = got, ref
    for k in OUTPUTS:
        if k in skip:
            assert not gb[k].any(), (k, "a skipped output was written")
        else:
            assert torch.equal(gb[k], rb[k]), k
    for k in rf["info"]:
        assert torch.equal(gf["info"][k], rf["info"][k]), ("info", k)
    assert np.array_equal(gf["rng"], rf["rng"]), "PCG64 words"
    assert gf["trackers"] == rf["trackers"], "tracker bytes"


def _key(tracker: dict | None):
    if tracker is None:
        return None
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in tracker.items()))


# ---------------------------------------------------------------------------------------------------------------- 1. step parity, no tracker
@pytest.mark.parametrize("n", [1, 32, 33, 70])
@pytest.mark.parametrize("pitch", [56, 64])
@pytest.mark.parametrize("hidden", [64, 128])
def test_step_parity_untracked(hidden, pitch, n):
    """n = 1: one lane; 32: a full tile; 33: a one-row second tile; 70: a partial third tile.  24 steps of 10-step episodes: every env
    auto-resets at least twice (asserted on the reference's done bytes).  One case each runs without value, log_prob, terminal_obs."""
    skip = {(64, 64, 33): ("value",), (128, 56, 70): ("log_prob",), (64, 56, 32): ("terminal_obs",)}.get((hidden, pitch, n), ())
    ref = _reference(hidden, pitch, n, 1, T_SPAN, None)
    resets = ((ref[0]["done"] & 3) != 0).sum(dim=0)
    assert int(resets.min()) >= 2, "an env of the reference reset fewer than twice"
    _assert_equal(_run(hidden, pitch, n, 1, T_SPAN, None, skip=skip), ref[:2], skip)


def test_single_step_span():
    """T = 1: the loop runs once; obs[1] is the only next observation"""
    ref = _reference(64, 64, 33, 1, 1, None)
    _assert_equal(_run(64, 64, 33, 1, 1, None), ref[:2])


def test_trained_scale_span():
    """the T4 policy of tests/trained_regime.py (saturated hidden units, sigma ~ 0.06), n = 33, T = 2: the same bit equality with the
    per-step path, and step 0 of the whole-rollout launch against an fp64 forward of obs[0]"""
    hidden, n = 64, 33
    ref = _reference(hidden, 64, n, 1, 2, None, regime="T4")
    got = _run(hidden, 64, n, 1, 2, None, regime="T4")
    _assert_equal(got, ref[:2])
    b = got[0]
    TR.assert_step_against_fp64(TR.trained_policy(hidden, 56, "T4", seed=hidden + n).flat, hidden, 56, b["obs"][0], _noise(2, n, n)[0],
                               {k: b[k][0] for k in ("value", "log_prob", "action")}, "step 0")


# ---------------------------------------------------------------------------------------------------------------- 2. tracker folded in, K = 1
def _tracker(n: int, initial: int = 1, max_stage: int | None = None) -> dict:
    """threshold 0: a promotion whenever the stage has seen min_episodes episodes and the window is full.  n >= 16: window 4, 6 episodes per
    stage, so that the n envs that truncate in one step promote in the middle of that step; n = 1: every episode promotes"""
    n_stages = _approach_cfg().n_stages
    return {"success_rate_threshold": 0.0, "window_episodes": 4 if n > 1 else 1, "min_episodes_per_stage": 6 if n > 1 else 1,
            "max_stage_index": n_stages - 1 if max_stage is None else max_stage, "initial": initial}


@pytest.mark.parametrize("n", [1, 16, 32])
def test_tracker_folded_in(n):
    """the workgroup that steps the envs replays their done bytes into the tracker.  On the reference: at least two promotions inside the span;
    for n > 1 at least one of them in the middle of a step's episodes (the stage's episode count after that step's observe is not 0: episodes
    of the same step came after the promotion; with one env a step has one episode and no middle); and a reset after a promotion sampled from
    the new stage (the env's stage_index plane holds a stage above the initial one)."""
    tr = _tracker(n)
    ref = _reference(64, 64, n, 1, T_SPAN, _key(tr))
    steps = ref[2]
    events = [s[0][0] for s in steps]
    assert events[-1] >= 2, "the reference tracker promoted fewer than twice"
    promoted_at = [t for t in range(T_SPAN) if events[t] > (events[t - 1] if t else 0)]
    if n > 1:
        assert any(steps[t][0][1] > 0 for t in promoted_at), "no promotion in the middle of a step's episodes"
    assert int(ref[1]["info"]["stage_index"].max()) > tr["initial"], "no reset sampled from a promoted stage"
    _assert_equal(_run(64, 64, n, 1, T_SPAN, tr), ref[:2])


def test_tracker_at_last_stage():
    """the tracker sits on its last stage: the window only records (ring, head, counts), nothing promotes"""
    tr = _tracker(16, initial=3, max_stage=3)
    ref = _reference(128, 56, 16, 1, T_SPAN, _key(tr))
    assert ref[2][-1][0][0] == 0 and ref[2][-1][0][2] == 3 and ref[2][-1][0][1] >= 32
    _assert_equal(_run(128, 56, 16, 1, T_SPAN, tr), ref[:2])


@pytest.mark.parametrize("split", [False, True])
def test_tracker_window_sum_carried(split):
    """The promotion test in double on a window sum that is not zero.  Window 20, 24 episodes per stage, threshold 0.2; before the span the
    tracker has seen 23 successful episodes (window full of ones, head 3, sum 20, count 23).  The 16 envs truncate at step 10 without success:
    the first of these episodes brings the count to 24 with rate 19 / 20 and promotes -- only if the kernel's window sum at its start is
    the 20 that the ring holds.  The promotion empties the window but leaves its ones in the ring, behind the 15 zeros of the rest of that
    step.  With ``split`` a second call starts at step 11 and rebuilds the sum from the ring: the five stale ones are not live, and
    counting them (sum 5, rate 0.25 once the window is full again at step 20) would promote a second time.  Asserted on the reference:
    exactly one promotion, at the step of the first truncations, and a sum that would have been wrong either way."""
    tr = {"success_rate_threshold": 0.2, "window_episodes": 20, "min_episodes_per_stage": 24, "max_stage_index": 7, "initial": 1, "preseed": 23}
    ref = _reference(64, 64, 16, 1, T_SPAN, _key(tr))
    steps = ref[2]
    first = next(t for t in range(T_SPAN) if steps[t][0][0] > 0)
    assert first == EPISODE_STEPS - 1 and steps[-1][0][0] == 1 and steps[-1][0][2] == 2, steps[-1]
    assert steps[first][0][1] == 15, "the promotion was not at the first episode of its step"
    spans = [(0, first + 2), (first + 2, T_SPAN - first - 2)] if split else None
    _assert_equal(_run(64, 64, 16, 1, T_SPAN, tr, spans=spans), ref[:2])


# ---------------------------------------------------------------------------------------------------------------- 3. population
def test_population_tracked():
    """K = 3 replicas x 16 envs on one handle with a PointCurriculumPopulation.  The population API shares threshold, window and
    min_episodes between its trackers; the replicas' stages diverge through their initial stages and the last stage: replica 0 starts on 0,
    replica 1 on 2, replica 2 on the last stage, where nothing promotes.  Asserted on the reference: three different stages at the end,
    different event counts.  The tracker bytes of every replica are compared."""
    n_stages = _approach_cfg().n_stages
    tr = {**_tracker(16), "initial": [0, 2, n_stages - 1]}
    ref = _reference(64, 64, 16, 3, T_SPAN, _key(tr))
    last = ref[2][-1]
    assert len({s[2] for s in last}) == 3 and last[0][0] >= 2 and last[1][0] >= 2 and last[2][0] == 0, last
    assert last[0][2] != 0 and last[1][2] != 2
    got = _run(64, 64, 16, 3, T_SPAN, tr)
    assert len(got[1]["trackers"]) == 3
    _assert_equal(got, ref[:2])


def test_population_untracked_bound():
    """a bound population handle with trackers == NULL (K = 2 x 40 envs: two tiles per replica, the second ragged): accepted; every replica
    resets on its own tracker's stage, which does not move"""
    from rl_brain_trainer_amd.curriculum import PointCurriculumPopulation

    def drive(whole: bool):
        env, _ = _make(2, 40, 64, None)
        cur = PointCurriculumPopulation(success_rate_threshold=0.0, window_episodes=4, min_episodes_per_stage=6, max_stage_index=7,
                                        initial_stage_indices=[1, 6])
        cur.attach(env)
        mlp = _mlp(64, 2, seed=5)
        b = _buffers(T_SPAN, 80, 64)
        noise = _noise(T_SPAN, 80, 5)
        b["obs"][0].copy_(env.reset())
        if whole:
            mlp.rollout_run(env, b["obs"], noise=noise, value=b["value"], action=b["action"], log_prob=b["log_prob"], reward=b["reward"],
                            done=b["done"], terminal_obs=b["terminal_obs"], first_step=0, n_steps=T_SPAN)
        else:
            for t in range(T_SPAN):
                mlp.forward_env_step(env, b["obs"][t], noise=noise[t], value=b["value"][t], action=b["action"][t], log_prob=b["log_prob"][t],
                                     next_obs=b["obs"][t + 1], reward=b["reward"][t], done=b["done"][t], terminal_obs=b["terminal_obs"][t])
        final = _final_state(env, cur, 2)
        mlp.close()
        cur.close()
        env.close()
        return b, final

    ref = drive(False)
    stages = ref[1]["info"]["stage_index"]
    # (a reset on stage s may sample one of the stages below it: the highest stage a replica's envs hold is its tracker's)
    assert int(stages[:40].max()) == 1 and int(stages[40:].max()) == 6
    _assert_equal(drive(True), ref)


# ---------------------------------------------------------------------------------------------------------------- 4. span splits
@pytest.mark.parametrize("tracked", [False, True])
def test_span_split(tracked):
    """[0, 24) against [0, 7) + [7, 24): buffers, env handle and tracker as after one call"""
    tr = _tracker(16) if tracked else None
    n = 16 if tracked else 33
    ref = _reference(64, 64, n, 1, T_SPAN, _key(tr))
    _assert_equal(_run(64, 64, n, 1, T_SPAN, tr, spans=[(0, 7), (7, T_SPAN - 7)]), ref[:2])


def test_span_above_the_cap():
    """a rollout of cap + 2 steps goes through the host's split (two kp1_rollout_run calls) and equals the per-step path; the entry point
    itself refuses n_steps = cap + 1"""
    from rl_brain_trainer_amd.mlp import span_split

    cap = native.ROLLOUT_RUN_MAX_STEPS
    T = cap + 2
    assert span_split(0, T, cap) == [(0, cap), (cap, 2)]
    ref = _reference(64, 64, 3, 1, T, None, 96)
    assert int(((ref[0]["done"] & 3) != 0).sum(dim=0).min()) >= 2
    _assert_equal(_run(64, 64, 3, 1, T, None, episode_steps=96), ref[:2])


# ---------------------------------------------------------------------------------------------------------------- 5. trainers
def _count_calls(monkeypatch) -> dict:
    from rl_brain_trainer_amd.mlp import MlpKernels

    calls = {"rollout_run": 0, "forward_env_step": 0}
    for name in calls:
        orig = getattr(MlpKernels, name)

        def counted(self, *args, _orig=orig, _name=name, **kwargs):
            calls[_name] += 1
            return _orig(self, *args, **kwargs)

        monkeypatch.setattr(MlpKernels, name, counted)
    return calls


def _trainer_state(ppo, env, trackers) -> dict:
    torch.cuda.synchronize()
    out = {name: getattr(ppo, name).clone() for name in TRAINER_BUFFERS}
    out.update(flat=ppo.flat.clone(), adam_m=ppo.adam_m.clone(), adam_v=ppo.adam_v.clone())
    out["rng"] = np.array(env.rng_state()).copy()
    out["trackers"] = [_bytes(t) for t in trackers]
    return out


def _same_states(a: list, b: list) -> None:
    for i, (x, y) in enumerate(zip(a, b)):
        for k in x:
            if isinstance(x[k], torch.Tensor):
                assert torch.equal(x[k], y[k]), (i, k)
            elif isinstance(x[k], np.ndarray):
                assert np.array_equal(x[k], y[k]), (i, k)
            else:
                assert x[k] == y[k], (i, k)


def _train_single(form: str, monkeypatch, *, n_envs: int = 16, hidden: int = 64, callback: bool = False):
    from rl_brain_trainer_amd.curriculum import PointCurriculum
    from rl_brain_trainer_amd.ppo import PPO, PPOConfig
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    monkeypatch.setenv("KP1_ROLLOUT_RUN", form)
    monkeypatch.setenv("KP1_FUSED_ROLLOUT", "1")      # the per-step path is the one-launch step: its calls are counted
    calls = _count_calls(monkeypatch)
    cfg = _approach_cfg(12)
    env = ArmKinematicVecEnv(cfg, n_envs, seed=21)
    cur = PointCurriculum(success_rate_threshold=0.0, window_episodes=4, min_episodes_per_stage=6, max_stage_index=cfg.n_stages - 1, initial_stage_index=2)
    ppo = PPO(env, PPOConfig(n_steps=32, batch_size=n_envs * 8, n_epochs=2, hidden=hidden, learning_rate=3e-4, seed=5), curriculum=cur)
    if callback:
        seen = []
        ppo.step_callback = lambda d: seen.append(1)
    whole = ppo._whole_rollout
    states = []
    for _ in range(2):                                 # graphs on: the first rollout captures, the second replays
        ppo.collect_rollouts()
        states.append(_trainer_state(ppo, env, [cur.read()]))
    ppo.train()
    states.append(_trainer_state(ppo, env, [cur.read()]))
    stage = int(cur.read().stage_index)
    assert bool(torch.isfinite(ppo.flat).all())
    ppo._mlp.close()
    cur.close()
    env.close()
    return states, dict(calls), stage, whole


def test_ppo_whole_rollout_equals_per_step(monkeypatch):
    """PPO(hidden=64, n_envs=16), a promoting PointCurriculum, graphs on: capture, one replay and one train() with KP1_ROLLOUT_RUN=1
    against 0 -- the flat parameters, the Adam moments, every rollout buffer, the env's random streams and the tracker"""
    s1, c1, stage1, w1 = _train_single("1", monkeypatch)
    s0, c0, stage0, w0 = _train_single("0", monkeypatch)
    assert w1 and not w0
    assert c1["rollout_run"] >= 2 and c1["forward_env_step"] == 0, c1      # warm-up + capture
    assert c0["rollout_run"] == 0 and c0["forward_env_step"] >= 32, c0
    assert stage1 == stage0 and stage1 > 2, "the tracker never promoted"
    _same_states(s1, s0)


def _train_population(form: str, monkeypatch):
    from rl_brain_trainer_amd.curriculum import PointCurriculumPopulation
    from rl_brain_trainer_amd.population import ApproachPopulationPPO
    from rl_brain_trainer_amd.ppo import PPOConfig
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    monkeypatch.setenv("KP1_ROLLOUT_RUN", form)
    monkeypatch.setenv("KP1_FUSED_ROLLOUT", "1")
    calls = _count_calls(monkeypatch)
    seeds, N = [7, 8], 16
    cfg = _approach_cfg(12)
    env = ArmKinematicPopulationVecEnv(cfg, seeds, N)
    cur = PointCurriculumPopulation(success_rate_threshold=0.0, window_episodes=4, min_episodes_per_stage=6, max_stage_index=cfg.n_stages - 1,
                                    initial_stage_indices=[0, 3])
    pop = ApproachPopulationPPO(seeds, PPOConfig(n_steps=32, batch_size=128, n_epochs=2, hidden=64, learning_rate=3e-4, ent_coef=1e-3), env, curriculum=cur)
    whole = pop._whole_rollout
    states = []
    for _ in range(2):
        pop.collect_rollouts()
        states.append(_trainer_state(pop, env, [cur.read(k) for k in range(2)]))
    pop.train()
    states.append(_trainer_state(pop, env, [cur.read(k) for k in range(2)]))
    stages = [int(cur.read(k).stage_index) for k in range(2)]
    pop._mlp.close()
    cur.close()
    env.close()
    return states, dict(calls), stages, whole


def test_approach_population_whole_rollout_equals_per_step(monkeypatch):
    """ApproachPopulationPPO (K = 2, N = 16), a promoting population tracker, graphs on: KP1_ROLLOUT_RUN=1 against 0"""
    s1, c1, st1, w1 = _train_population("1", monkeypatch)
    s0, c0, st0, w0 = _train_population("0", monkeypatch)
    assert w1 and not w0
    assert c1["rollout_run"] >= 2 and c1["forward_env_step"] == 0, c1
    assert c0["rollout_run"] == 0 and c0["forward_env_step"] >= 32, c0
    assert st1 == st0 and st1[0] > 0 and st1[1] > 3, st1
    _same_states(s1, s0)


@pytest.mark.parametrize("case", ["step_callback", "tracked_40_envs", "hidden_256"])
def test_fallbacks_take_the_per_step_path(case, monkeypatch):
    """with KP1_ROLLOUT_RUN=1: a step callback, 40 envs with a tracker and hidden 256 take the per-step path and still train"""
    kw = {"step_callback": {"callback": True}, "tracked_40_envs": {"n_envs": 40}, "hidden_256": {"hidden": 256}}[case]
    _, calls, _, whole = _train_single("1", monkeypatch, **kw)
    assert not whole and calls["rollout_run"] == 0 and calls["forward_env_step"] >= 32, calls


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def _raw(mlp, env_handle, a: dict, *, n_steps: int = 2, stride: int | None = None, trackers=None):
    L = native.load()
    L.kp1_last_error.restype = C.c_char_p
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    rc = L.kp1_rollout_run(mlp._h, env_handle, p(a["obs"]), a["obs"].shape[2] if stride is None else stride, p(a["noise"]), p(a["value"]),
                           p(a["action"]), p(a["log_prob"]), p(a["reward"]), p(a["done"]), p(a["terminal_obs"]), n_steps,
                           C.c_void_p(trackers) if trackers else None, 12, mlp._stream())
    return rc, L.kp1_last_error().decode(errors="replace")


def _marked(T: int, rows: int, w: int) -> dict:
    f = lambda *shape, v=-7.5: torch.full(shape, v, dtype=torch.float32, device=DEV)   # noqa: E731
    return {"obs": f(T + 1, rows, w), "noise": f(T, rows, 7, v=0.0), "value": f(T, rows), "action": f(T, rows, 7), "log_prob": f(T, rows),
            "reward": f(T, rows), "done": torch.full((T, rows), 200, dtype=torch.uint8, device=DEV), "terminal_obs": f(T, rows, w)}


def _untouched(a: dict) -> bool:
    torch.cuda.synchronize()
    return all(bool((a[k] == (200 if k == "done" else -7.5)).all()) for k in OUTPUTS if a[k] is not None)


def test_refusals():
    """every refusal of kp1_rollout_run, before any launch: status, kp1_last_error text, outputs untouched"""
    from rl_brain_trainer_amd import finisher_tools as ft
    from rl_brain_trainer_amd.curriculum import PointCurriculum, PointCurriculumPopulation
    from rl_brain_trainer_amd.mlp import MlpKernels
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    acfg = _approach_cfg()
    mlp = _mlp(64, 1, seed=1)
    env = ArmKinematicVecEnv(acfg, 12, seed=1)
    env.set_obs_stride(64)
    env.reset()
    rng0 = np.array(env.rng_state()).copy()

    def refused(m, handle, args, status, text, **kw):
        rc, msg = _raw(m, handle, args, **kw)
        assert rc == status and text in msg, (rc, msg)
        assert _untouched(args), text

    a = _marked(2, 12, 64)
    # NULL required arguments, noise included
    for key in ("obs", "noise", "action", "reward", "done"):
        b = dict(a)
        b[key] = None
        L = native.load()
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        rc = L.kp1_rollout_run(mlp._h, env._handle, p(b["obs"]), 64, p(b["noise"]), p(b["value"]), p(b["action"]), p(b["log_prob"]), p(b["reward"]),
                               p(b["done"]), p(b["terminal_obs"]), 2, None, 12, mlp._stream())
        assert rc == KP1_ERR_INVALID and "NULL argument" in L.kp1_last_error().decode(), key
        assert _untouched(a), key
    # n_steps
    refused(mlp, env._handle, a, KP1_ERR_INVALID, "KP1_ROLLOUT_RUN_MAX_STEPS", n_steps=0)
    refused(mlp, env._handle, a, KP1_ERR_INVALID, "KP1_ROLLOUT_RUN_MAX_STEPS", n_steps=native.ROLLOUT_RUN_MAX_STEPS + 1)
    # obs_stride: neither 56 nor 64; not the env handle's pitch
    refused(mlp, env._handle, a, KP1_ERR_INVALID, "obs_stride must be 56 or 64", stride=60)
    refused(mlp, env._handle, a, KP1_ERR_INVALID, "observation pitch", stride=56)
    # terminal_obs overlapping the obs buffer
    big = torch.full((5, 12, 64), -7.5, dtype=torch.float32, device=DEV)
    refused(mlp, env._handle, {**a, "obs": big[:3], "terminal_obs": big[2:4]}, KP1_ERR_INVALID, "must not overlap the obs buffer")
    # hidden 256; the 80-float observation
    m256 = MlpKernels(256, DEV, max_batch=64)
    refused(m256, env._handle, a, KP1_ERR_UNSUPPORTED, "hidden 256")
    m256.close()
    m80 = MlpKernels(64, DEV, max_batch=128, obs_dim=80)
    refused(m80, env._handle, a, KP1_ERR_UNSUPPORTED, "56-float observation", stride=128)
    m80.close()
    # recorded reward components; f64 handles
    env.enable_reward_components(True)
    refused(mlp, env._handle, a, KP1_ERR_UNSUPPORTED, "reward components")
    env.enable_reward_components(False)
    e64 = ArmKinematicVecEnv(acfg, 12, seed=1, real="f64")
    refused(mlp, e64._handle, a, KP1_ERR_UNSUPPORTED, "fp32 handle")
    e64.close()
    # the dock mode, and a handle bound to dock stage records
    denv = ArmKinematicVecEnv(load_golden_config(DOCK_CFG), 12, seed=1)
    denv.set_obs_stride(64)
    refused(mlp, denv._handle, a, KP1_ERR_UNSUPPORTED, "dock mode")
    denv.close()
    m2 = _mlp(64, 2, seed=2)
    dpop = ArmKinematicPopulationVecEnv(load_golden_config(DOCK_CFG), [1, 2], 6, mode="dock")
    stages = [{"name": "close", "min_episodes": 6, "window_episodes": 4, "success_rate_threshold": 0.0, "dock_residual_action_limit": 0.2,
               "close_bucket_probability": 1.0, "close_bucket_max_pos_error_m": 0.003, "handoff_state_probability": 0.3, "init_q_noise": [0.002] * 7},
              {"name": "wide", "dock_delta_q_change_limit_scale": 0.5, "dock_residual_action_limit": 0.35, "close_bucket_probability": 0.1,
               "handoff_state_probability": 0.9, "handoff_state_max_action_l2": 0.5}]
    dcur = ft.DockReverseCurriculumPopulation(stages=stages, window_episodes=4, n_replicas=2, handoff_base_dirs=(GOLDEN,))
    dcur.attach(dpop)
    dpop.set_obs_stride(64)
    refused(m2, dpop._handle, a, KP1_ERR_UNSUPPORTED, "dock stage records")
    dcur.close()
    dpop.close()
    # the env count is no multiple of K; a bound population of another replica count
    e13 = ArmKinematicVecEnv(acfg, 13, seed=1)
    e13.set_obs_stride(64)
    refused(m2, e13._handle, _marked(2, 13, 64), KP1_ERR_INVALID, "multiple of the handle's replica count")
    e13.close()
    penv = ArmKinematicPopulationVecEnv(acfg, [1, 2, 3], 4)
    pcur = PointCurriculumPopulation(success_rate_threshold=0.5, window_episodes=4, min_episodes_per_stage=4, max_stage_index=acfg.n_stages - 1,
                                     initial_stage_indices=[0, 1, 2])
    pcur.attach(penv)
    penv.set_obs_stride(64)
    refused(m2, penv._handle, a, KP1_ERR_INVALID, "replica count differs")
    refused(mlp, penv._handle, a, KP1_ERR_INVALID, "replica count differs")
    # trackers that are not the handle's bound stage source: an unbound handle, a tracker the handle is not attached to, a population's other
    other = PointCurriculum(success_rate_threshold=0.5, window_episodes=4, min_episodes_per_stage=4, max_stage_index=3)
    mine = PointCurriculum(success_rate_threshold=0.5, window_episodes=4, min_episodes_per_stage=4, max_stage_index=3)
    refused(mlp, env._handle, a, KP1_ERR_INVALID, "bound stage source", trackers=other.device_state)
    mine.attach(env)
    refused(mlp, env._handle, a, KP1_ERR_INVALID, "bound stage source", trackers=other.device_state)
    m3 = _mlp(64, 3, seed=3)
    refused(m3, penv._handle, a, KP1_ERR_INVALID, "bound stage source", trackers=other.device_state)
    m3.close()
    # a negative steps_per_call with trackers
    L = native.load()
    rc = L.kp1_rollout_run(mlp._h, env._handle, *[C.c_void_p(a[k].data_ptr()) if k != "stride" else 64 for k in ("obs", "stride", "noise", "value", "action",
                           "log_prob", "reward", "done", "terminal_obs")], 2, C.c_void_p(mine.device_state), -1, mlp._stream())
    assert rc == KP1_ERR_INVALID and "steps_per_call is negative" in L.kp1_last_error().decode() and _untouched(a)
    # trackers with more than 32 envs per replica
    e40 = ArmKinematicVecEnv(acfg, 40, seed=1)
    e40.set_obs_stride(64)
    t40 = PointCurriculum(success_rate_threshold=0.5, window_episodes=4, min_episodes_per_stage=4, max_stage_index=3)
    t40.attach(e40)
    refused(mlp, e40._handle, _marked(2, 40, 64), KP1_ERR_UNSUPPORTED, "at most 32 envs per replica", trackers=t40.device_state)
    assert _bytes(t40.read()) == _bytes(other.read()), "a refused call moved the tracker"
    t40.close()
    e40.close()
    # nothing above moved the env or the bound tracker
    assert np.array_equal(np.array(env.rng_state()), rng0)
    assert _bytes(mine.read()) == _bytes(other.read())
    for obj in (other, mine, pcur, penv, m2):
        obj.close()

    # route envs have no kp1_env step of their own: refused on the host
    class NotAnArmEnv:
        n_envs, _handle = 12, env._handle

    with pytest.raises(TypeError, match="route envs"):
        mlp.rollout_run(NotAnArmEnv(), a["obs"], **{k: v for k, v in a.items() if k != "obs"}, first_step=0, n_steps=2)
    assert _untouched(a)
    # different devices: needs a second GPU; on a one-GPU machine say so in the test report
    if torch.cuda.device_count() > 1:
        m_other = MlpKernels(64, torch.device("cuda", 1), max_batch=128)
        refused(m_other, env._handle, a, KP1_ERR_INVALID, "different devices")
        m_other.close()
    else:
        warnings.warn("kp1_rollout_run's different-devices refusal was not exercised: this machine has one GPU")
    mlp.close()
    env.close()
