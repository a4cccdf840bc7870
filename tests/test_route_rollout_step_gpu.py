"""One-launch rollout step of the route envs (kp1_mlp_forward_route_step, route_rollout_step_kernel), on the GPU: bit for bit the launch
sequence kp1_mlp_forward + kp1_route_step on a twin env -- single handles at both observation widths and pitches, populations with promoting
prefix trackers, and the two trainers that use it (graphs on).  Every comparison is torch.equal / np.array_equal.

The config is the golden route config with episodes of at most 12 steps and the route-ready test reduced to the action norm (the other four
thresholds at 1e3, the action threshold at 0.68).  The test policy's actions are ~ 0.37 N(0, 1) per joint, so an env is route-ready in about
one step of seven whatever its state: waypoint successes, sequence advances, sequence successes and truncations all occur every few episodes.
Chosen on the CPU oracle (oracle/route_oracle.py, 40 envs x 100 steps of such actions): with `sequence` on every single env saw >= 11 waypoint
successes, >= 7 advances, >= 3 sequence successes, >= 2 truncations and >= 9 resets.  The tests count these on the launch-sequence twin and
fail when one is missing."""
from __future__ import annotations

import ctypes as C
import json
import warnings

import numpy as np
import pytest
import torch

import trained_regime as T
from conftest import GOLDEN
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import route_config as rcfg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KP1_ERR_INVALID, KP1_ERR_UNSUPPORTED = -1, -4     # include/kp1.h
TERMINATED, TRUNCATED, SUCCESS = 1, 2, 4          # KP1_DONE_*
STEPS, MAX_EPISODE_STEPS, ACTION_THRESHOLD = 100, 12, 0.68
BUFFERS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "adv_buf", "ret_buf", "term_obs_buf")


def _cfg(sequence: bool = True, route_keys: bool = True) -> dict:
    cfgd = json.loads((GOLDEN / "configs" / "route_curriculum_prefix120_routeobs_sequence2.json").read_text())
    cfgd["route"].setdefault("sequence", {})["enabled"] = sequence
    cfgd["route"].setdefault("observation", {})["include_route_keys"] = route_keys
    cfgd["env"]["termination"]["max_episode_steps"] = MAX_EPISODE_STEPS
    cfgd["route"]["reward"].update(route_ready_q_threshold=1e3, route_ready_pos_threshold_m=1e3, route_ready_ori_threshold_rad=1e3,
                                   route_ready_dq_threshold=1e3, route_ready_action_threshold=ACTION_THRESHOLD)
    return cfgd


def _route_q() -> np.ndarray:
    return rcfg.load_route_q(GOLDEN / "synthetic_route.json")


def _single_env(cfgd: dict, n: int, pitch: int, *, seed: int = 31, real: str = "f32", route_q: np.ndarray | None = None):
    from rl_brain_trainer_amd.route_env import RouteVecEnv

    env = RouteVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=40), _route_q() if route_q is None else route_q,
                      n, seed=seed, real=real)
    env.set_obs_stride(pitch)
    return env


def _bytes(obj) -> bytes:
    return bytes(C.string_at(C.addressof(obj), C.sizeof(obj)))


def _mlp(hidden: int, K: int, obs_dim: int, seed: int, max_batch: int = 128, regime: str | None = None):
    """a K-replica handle with [K, P] parameters: orthogonal weights, an action head large enough for the mean to matter (means of a few
    hundredths), random biases, log_std near -1 (the action-norm distribution the route-ready threshold was chosen for).  ``regime``: the
    trained-scale policies of tests/trained_regime.py in their place (another action-norm distribution)"""
    from rl_brain_trainer_amd.mlp import MlpKernels
    from rl_brain_trainer_amd.ppo import ActorCritic

    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    rows = []
    for k in range(K):
        if regime is not None:
            rows.append(T.trained_policy(hidden, obs_dim, regime, seed=seed + k).flat.to(DEV))
            continue
        pol = ActorCritic(hidden, DEV, seed=seed + k, obs_dim=obs_dim)
        pol.views["action_net.weight"].mul_(5.0)
        for name, v in pol.views.items():
            if name.endswith("bias"):
                v.copy_((torch.rand(v.shape, generator=g) * 0.1 - 0.05).to(DEV))
        pol.views["log_std"].copy_((-1.0 + 0.1 * (torch.rand(7, generator=g) - 0.5)).to(DEV))
        rows.append(pol.flat.clone())
    flat = torch.stack(rows).contiguous()
    mlp = MlpKernels(hidden, DEV, max_batch=max_batch, obs_dim=obs_dim, replicas=K)
    mlp.pack(flat if K > 1 else flat[0].contiguous())
    return mlp


def _step_parity(mlp, env_a, env_b, n_per_replica: int, *, sequence: bool, after_a=None, after_b=None, with_value: bool = True,
                 with_log_prob: bool = True, with_terminal_obs: bool = True, seed: int = 0, fp64_flat: torch.Tensor | None = None) -> None:
    """Twin A takes forward_route_step, twin B forward + step_into(auto_reset=True), on the same weights and noise: every output of every
    step (whole buffers, padding columns included), then every info plane (route and base) and both PCG64 streams.  ``after_*``: the tracker
    launch that follows a step.  The branch counts are taken on twin B, per 32-row tile of each replica.  ``fp64_flat`` (K = 1): the
    parameters of a trained-scale policy, for a check of step 0's value, log_prob and unclipped action against an fp64 forward of the
    observations the env holds at that step; its actions are not the ones the route-ready threshold was chosen for, so of the branch
    conditions only the resets are required of it."""
    n, w = env_a.n_envs, env_a.obs_stride
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=DEV)   # noqa: E731
    obs_a, obs_b = env_a.reset().clone(), env_b.reset().clone()
    assert obs_a.shape == (n, w) and torch.equal(obs_a, obs_b)
    gen = torch.Generator(device=DEV).manual_seed(99 + seed)
    counts = {k: z(n, dt=torch.int64) for k in ("waypoint_success", "advance", "sequence_success", "truncation", "reset")}
    for t in range(STEPS):
        noise = torch.randn((n, 7), generator=gen, device=DEV)
        a = {"value": z(n), "action": z(n, 7), "log_prob": z(n), "next_obs": z(n, w), "reward": z(n), "done": z(n, dt=torch.uint8),
             "terminal_obs": z(n, w)}
        b = {k: torch.zeros_like(v) for k, v in a.items()}
        clipped = z(n, 7)
        mlp.forward_route_step(env_a, obs_a, noise=noise, value=a["value"] if with_value else None, action=a["action"],
                               log_prob=a["log_prob"] if with_log_prob else None, next_obs=a["next_obs"], reward=a["reward"], done=a["done"],
                               terminal_obs=a["terminal_obs"] if with_terminal_obs else None)
        mlp.forward(obs_b, noise=noise, value=b["value"], action=b["action"], clipped=clipped, log_prob=b["log_prob"])
        env_b.step_into(clipped, b["next_obs"], b["reward"], b["done"], b["terminal_obs"] if with_terminal_obs else None, True)
        if after_a is not None:
            after_a(a["done"])
            after_b(b["done"])
        if not with_value:
            assert not a["value"].any()
            b["value"].zero_()
        if not with_log_prob:
            assert not a["log_prob"].any()
            b["log_prob"].zero_()
        for k in a:
            assert torch.equal(a[k], b[k]), (t, k)
        if fp64_flat is not None and t == 0:
            T.assert_step_against_fp64(fp64_flat, mlp.hidden, mlp.obs_dim, obs_a, noise, {k: a[k] for k in ("value", "log_prob", "action")}, "step 0")
        done = b["done"]
        wp = env_b.info()["route_waypoint_success"].ne(0)
        term, trunc = (done & TERMINATED).ne(0), (done & TRUNCATED).ne(0)
        counts["waypoint_success"] += wp
        counts["advance"] += wp & ~term
        counts["sequence_success"] += (done & SUCCESS).ne(0)
        counts["truncation"] += trunc & ~term
        counts["reset"] += term | trunc
        if with_terminal_obs:      # the terminal observation of a finished env is a real row, an unfinished env's stays unwritten
            fin = term | trunc
            assert bool(b["terminal_obs"][fin].abs().sum(1).gt(0).all()) and not b["terminal_obs"][~fin].any()
        obs_a, obs_b = a["next_obs"], b["next_obs"]
    ia, ib = env_a.info(), env_b.info()
    for k in ib:
        assert torch.equal(ia[k], ib[k]), k
    assert np.array_equal(env_a.rng_state(), env_b.rng_state())                     # the wrapper's streams (kp1_route_rng_get)
    assert np.array_equal(env_a.base.rng_state(), env_b.base.rng_state())           # the base env's (kp1_rng_get)
    # branch coverage is a condition: overall, and with `sequence` on in every tile of every replica
    assert int(counts["reset"].min()) >= 2, "an env auto-reset fewer than twice"
    if fp64_flat is not None:
        return
    needed = ("waypoint_success", "advance", "sequence_success", "truncation") if sequence else ("waypoint_success", "truncation")
    for name in needed:
        assert int(counts[name].sum()) > 0, f"no {name} in the run"
    if sequence:
        for r0 in range(0, n, n_per_replica):
            for t0 in range(r0, r0 + n_per_replica, 32):
                for name in needed:
                    assert int(counts[name][t0:min(t0 + 32, r0 + n_per_replica)].sum()) > 0, f"no {name} in the tile of env {t0}"
    else:
        assert int(counts["advance"].sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- 1. single handles
# (hidden, obs_dim, pitch, sequence, E): every value of every axis with E = 33 (a tile plus one row) and with E = 70 (three tiles, the last
# ragged); E = 1 one live row; E = 32 one exact tile
SINGLE_CASES = [
    (64, 80, 80, True, 33), (128, 80, 128, False, 33), (128, 56, 56, True, 33), (64, 56, 64, False, 33),
    (128, 80, 80, False, 70), (64, 80, 128, True, 70), (64, 56, 56, False, 70), (128, 56, 64, True, 70),
    (64, 80, 128, True, 1), (128, 56, 64, True, 1), (128, 80, 128, True, 32), (64, 56, 56, False, 32),
]


@pytest.mark.parametrize("hidden,obs_dim,pitch,sequence,E", SINGLE_CASES)
def test_step_parity_single(hidden, obs_dim, pitch, sequence, E):
    """one case runs without the value plane, one without log_prob, one without terminal_obs"""
    cfgd = _cfg(sequence, obs_dim == 80)
    envs = [_single_env(cfgd, E, pitch) for _ in range(2)]
    assert envs[0].obs_dim == obs_dim
    mlp = _mlp(hidden, 1, obs_dim, seed=hidden + E)
    case = (hidden, obs_dim, pitch, sequence, E)
    _step_parity(mlp, envs[0], envs[1], E, sequence=sequence, with_value=case != (64, 80, 80, True, 33),
                 with_log_prob=case != (128, 80, 80, False, 70), with_terminal_obs=case != (64, 56, 56, False, 70), seed=E)
    mlp.close()
    for env in envs:
        env.close()


def test_step_parity_trained_scale():
    """the T4 policy of tests/trained_regime.py (saturated hidden units, sigma ~ 0.06) on the 80-float observation at pitch 128, E = 33: the
    same bit equality over every step, and step 0 against fp64"""
    cfgd = _cfg(True, True)
    envs = [_single_env(cfgd, 33, 128) for _ in range(2)]
    mlp = _mlp(128, 1, 80, seed=3, regime="T4")
    _step_parity(mlp, envs[0], envs[1], 33, sequence=True, seed=33, fp64_flat=T.trained_policy(128, 80, "T4", seed=3).flat)
    mlp.close()
    for env in envs:
        env.close()


# ---------------------------------------------------------------------------------------------------------------- 2. populations
def _tracker_kwargs(prefixes=(10, 20, 30, 40), episodes: int = 12) -> dict:
    from rl_brain_trainer_amd.route_curriculum import build_prefix_stages

    return dict(stages=build_prefix_stages(list(prefixes)), promotion_success_rate=0.0, promotion_route_ready_hit_rate=0.0,
                promotion_orientation_hit_rate=0.0, promotion_max_regression_rate=1.0, window_episodes=episodes, min_episodes_per_stage=episodes)


@pytest.mark.parametrize("hidden,N,route_keys", [(64, 16, True), (128, 40, True), (64, 40, False)])
def test_step_parity_population(hidden, N, route_keys):
    """K = 3 replicas on one RoutePopulationVecEnv with a RoutePrefixCurriculumPopulation that promotes on every 12 finished episodes
    (thresholds 0), against the launch sequence on a twin population: N = 16 a half-empty tile per replica, N = 40 a ragged second tile.  The
    auto-reset of env i reads the window of replica i / N, which the tracker moves."""
    from rl_brain_trainer_amd.route_curriculum import RoutePrefixCurriculumPopulation
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv

    seeds = [11, 12, 40]
    cfgd = _cfg(True, route_keys)
    obs_dim = 80 if route_keys else 56
    envs, curs = [], []
    for _ in range(2):
        env = RoutePopulationVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=40), _route_q(), seeds, N)
        cur = RoutePrefixCurriculumPopulation(**_tracker_kwargs())
        cur.attach(env)
        env.set_obs_stride(128 if route_keys else 64)
        envs.append(env)
        curs.append(cur)
    first = [tuple(int(v) for v in _window(curs[0], envs[0], k)) for k in range(3)]
    mlp = _mlp(hidden, 3, obs_dim, seed=hidden + N)
    _step_parity(mlp, envs[0], envs[1], N, sequence=True, after_a=lambda d: curs[0].observe(d, N), after_b=lambda d: curs[1].observe(d, N), seed=N)
    for k in range(3):
        sa, sb = curs[0].read(k), curs[1].read(k)
        assert _bytes(sa) == _bytes(sb), k
        assert int(sa.stage_index) > 0, (k, "the replica never promoted")
        assert envs[0].window(k) == envs[1].window(k) != first[k], (k, "the replica's window never moved")
    mlp.close()
    for cur, env in zip(curs, envs):
        cur.close()
        env.close()


def _window(cur, env, k):
    cur.read(k)          # brings the host copy of window k up to date
    return env.window(k)


# ---------------------------------------------------------------------------------------------------------------- 3. trainers
T_STEPS, N_ENVS = 8, 16


def _count_route_calls(monkeypatch) -> list[int]:
    from rl_brain_trainer_amd.mlp import MlpKernels

    calls = [0]
    orig = MlpKernels.forward_route_step

    def counted(self, *args, **kwargs):
        calls[0] += 1
        return orig(self, *args, **kwargs)

    monkeypatch.setattr(MlpKernels, "forward_route_step", counted)
    return calls


def _trainer_state(ppo, env, trackers) -> dict:
    torch.cuda.synchronize()
    out = {name: getattr(ppo, name).clone() for name in BUFFERS}
    out.update(flat=ppo.flat.clone(), adam_m=ppo.adam_m.clone(), adam_v=ppo.adam_v.clone())
    out["rng"], out["base_rng"] = env.rng_state(), env.base.rng_state()
    out["trackers"] = [_bytes(t) for t in trackers]
    return out


def _assert_same(a: dict, b: dict, what) -> None:
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), (what, k)
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k)


def _run_trainer(kind: str, switch: str | None, monkeypatch, toggle_components: bool = False):
    """``kind``: "population" (RoutePopulationPPO, K = 2) or "single" (PPO on a RouteVecEnv); N = 16, T = 8, one epoch, graphs on.  Rollouts:
    capture, replay (after the optional reward-component toggle: a re-capture), then one train()."""
    from rl_brain_trainer_amd.population import RoutePopulationPPO
    from rl_brain_trainer_amd.ppo import PPO, PPOConfig
    from rl_brain_trainer_amd.route_curriculum import RoutePrefixCurriculumDevice, RoutePrefixCurriculumPopulation
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv, RouteVecEnv

    monkeypatch.delenv("KP1_FUSED_ROLLOUT", raising=False)
    if switch is None:
        monkeypatch.delenv("KP1_FUSED_ROUTE_ROLLOUT", raising=False)
    else:
        monkeypatch.setenv("KP1_FUSED_ROUTE_ROLLOUT", switch)
    calls = _count_route_calls(monkeypatch)
    cfgd = _cfg()
    env_cfg, route_cfg = kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=10)
    pcfg = PPOConfig(n_steps=T_STEPS, batch_size=64, n_epochs=1, hidden=64, learning_rate=3e-4, ent_coef=1e-3, seed=5)
    if kind == "population":
        seeds = [7, 8]
        env = RoutePopulationVecEnv(env_cfg, route_cfg, _route_q(), seeds, N_ENVS)
        cur = RoutePrefixCurriculumPopulation(**_tracker_kwargs((10, 20, 30), 8))
        ppo = RoutePopulationPPO(seeds, pcfg, env, curriculum=cur)
        read = lambda: [cur.read(k) for k in range(2)]   # noqa: E731
    else:
        env = RouteVecEnv(env_cfg, route_cfg, _route_q(), N_ENVS, seed=7)
        cur = RoutePrefixCurriculumDevice(**_tracker_kwargs((10, 20, 30), 8))
        ppo = PPO(env, pcfg, curriculum=cur)
        read = lambda: [cur.read()]   # noqa: E731
    on = switch is not None and switch != "0"
    assert ppo.use_graphs and ppo._fused_route_step == on and not ppo._fused_env_step
    states, counts = [], []
    for it in range(3 if toggle_components else 2):
        if toggle_components and it == 1:
            env.enable_reward_components(True)               # the next rollout re-captures, as forward + step_into
            assert not ppo._fused_route_step
        ppo.collect_rollouts()
        states.append(_trainer_state(ppo, env, read()))
        counts.append(calls[0])
    ppo.train()
    states.append(_trainer_state(ppo, env, read()))
    ppo._mlp.close()
    cur.close()
    env.close()
    return states, counts


@pytest.mark.parametrize("kind", ["population", "single"])
def test_trainers_route_rollout_equals_launch_sequence(kind, monkeypatch):
    """KP1_FUSED_ROUTE_ROLLOUT=1 against unset over capture, replay and one train(): rollout buffers, flat parameters, Adam moments, both
    random streams and the tracker bytes.  With the switch the first rollout goes through forward_route_step T times (plus the one warm-up
    step before the capture) and the replay launches the captured graph; without it, never."""
    s1, c1 = _run_trainer(kind, "1", monkeypatch)
    s0, c0 = _run_trainer(kind, None, monkeypatch)
    assert c1 == [T_STEPS + 1, T_STEPS + 1] and c0 == [0, 0], (c1, c0)
    for i, (x, y) in enumerate(zip(s1, s0)):
        _assert_same(x, y, i)
    assert bool((s0[1]["done_buf"] & 3).ne(0).any()), "no episode ended in the compared rollouts"


@pytest.mark.parametrize("kind", ["population", "single"])
def test_trainers_reward_components_toggled_after_construction(kind, monkeypatch):
    """enable_reward_components(True) after the first rollout: the re-captured rollout falls back to forward + step_into and equals an unset
    run that made the same toggle"""
    s1, c1 = _run_trainer(kind, "1", monkeypatch, toggle_components=True)
    s0, c0 = _run_trainer(kind, None, monkeypatch, toggle_components=True)
    assert c1 == [T_STEPS + 1] * 3 and c0 == [0] * 3, (c1, c0)      # no one-launch step after the toggle
    for i, (x, y) in enumerate(zip(s1, s0)):
        _assert_same(x, y, i)


def test_eager_rollout_takes_the_route_form_every_step(monkeypatch):
    """graphs off: T calls of forward_route_step per rollout with the switch"""
    from rl_brain_trainer_amd.ppo import PPO, PPOConfig

    monkeypatch.setenv("KP1_FUSED_ROUTE_ROLLOUT", "1")
    calls = _count_route_calls(monkeypatch)
    env = _single_env(_cfg(), N_ENVS, 80, seed=7)
    ppo = PPO(env, PPOConfig(n_steps=T_STEPS, batch_size=64, n_epochs=1, hidden=128, seed=5), use_graphs=False)
    for it in range(2):
        ppo.collect_rollouts()
        assert calls[0] == (it + 1) * T_STEPS
    ppo._mlp.close()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def _raw_call(mlp, env_handle, *, obs, noise, value, action, log_prob, next_obs, reward, done, terminal_obs, stride=None):
    L = native.load()
    L.kp1_last_error.restype = C.c_char_p
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    rc = L.kp1_mlp_forward_route_step(mlp._h, env_handle, p(obs), obs.shape[1] if stride is None else stride, p(noise), p(value), p(action),
                                      p(log_prob), p(next_obs), p(reward), p(done), p(terminal_obs), mlp._stream())
    return rc, L.kp1_last_error().decode(errors="replace")


def _marked(n: int, w: int) -> dict:
    """call arguments whose outputs carry a marker, so that a refused call can be seen to have written nothing"""
    f = lambda *shape, v=0.0: torch.full(shape, v, dtype=torch.float32, device=DEV)   # noqa: E731
    return {"obs": f(n, w), "noise": f(n, 7), "value": f(n, v=-7.5), "action": f(n, 7, v=-7.5), "log_prob": f(n, v=-7.5),
            "next_obs": f(n, w, v=-7.5), "reward": f(n, v=-7.5), "done": torch.full((n,), 200, dtype=torch.uint8, device=DEV),
            "terminal_obs": f(n, w, v=-7.5)}


def _untouched(args: dict) -> bool:
    """(an output that shares its storage with obs carries no marker: the call was refused for it, and the caller checks that storage)"""
    torch.cuda.synchronize()
    base = args["obs"].untyped_storage().data_ptr()
    outs = [(k, args[k]) for k in ("value", "action", "log_prob", "next_obs", "reward", "done", "terminal_obs")
            if args[k] is not None and args[k].untyped_storage().data_ptr() != base]
    return all(bool((t == (200 if k == "done" else -7.5)).all()) for k, t in outs)


def test_refusals():
    """every refusal of kp1_mlp_forward_route_step, before any launch: status, kp1_last_error text, outputs untouched.  (An env count that is
    no multiple of K cannot be built through the ABI: kp1_route_create_population refuses it, and the replica counts are compared first.)"""
    from rl_brain_trainer_amd.mlp import MlpKernels
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    n = 12
    cfgd = _cfg(False, True)
    env = _single_env(cfgd, n, 128)
    env.reset()
    mlp = _mlp(64, 1, 80, seed=1)

    def refused(m, handle, args, status, text, **kw):
        rc, msg = _raw_call(m, handle, **args, **kw)
        assert rc == status and text in msg, (rc, msg)
        assert _untouched(args), text

    a = _marked(n, 128)
    # NULL required arguments, noise included
    for key in ("noise", "action", "next_obs", "reward", "done"):
        refused(mlp, env._handle, {**a, key: None}, KP1_ERR_INVALID, "NULL argument")
    L = native.load()
    assert L.kp1_mlp_forward_route_step(mlp._h, env._handle, None, 128, None, None, None, None, None, None, None, None, None) == KP1_ERR_INVALID
    assert L.kp1_mlp_forward_route_step(mlp._h, None, C.c_void_p(a["obs"].data_ptr()), 128, None, None, None, None, None, None, None, None,
                                        None) == KP1_ERR_INVALID
    # hidden 256
    m256 = MlpKernels(256, DEV, max_batch=64, obs_dim=80)
    refused(m256, env._handle, a, KP1_ERR_UNSUPPORTED, "hidden 256")
    m256.close()
    # obs_dim of the two handles
    m56 = _mlp(64, 1, 56, seed=2)
    refused(m56, env._handle, _marked(n, 64), KP1_ERR_INVALID, "obs_dim differs")
    m56.close()
    # obs_stride: neither the width nor the padded width; not the route handle's
    refused(mlp, env._handle, a, KP1_ERR_INVALID, "obs_stride must be", stride=100)
    refused(mlp, env._handle, _marked(n, 80), KP1_ERR_INVALID, "differs from the route handle's")
    # recorded route reward components
    env.enable_reward_components(True)
    refused(mlp, env._handle, a, KP1_ERR_UNSUPPORTED, "route reward components")
    env.enable_reward_components(False)
    # a live chain
    chain = env.chain(1, 3)
    refused(mlp, env._handle, a, KP1_ERR_UNSUPPORTED, "live kp1_route_chain")
    chain.close()
    # replica counts
    m2 = _mlp(64, 2, 80, seed=3)
    refused(m2, env._handle, a, KP1_ERR_INVALID, "replica count differs")
    penv = RoutePopulationVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=40), _route_q(), [1, 2, 3], 4)
    penv.set_obs_stride(128)
    refused(m2, penv._handle, a, KP1_ERR_INVALID, "replica count differs")
    refused(mlp, penv._handle, a, KP1_ERR_INVALID, "replica count differs")
    penv.close()
    m2.close()
    # next_obs == obs, partial overlaps
    refused(mlp, env._handle, {**a, "next_obs": a["obs"]}, KP1_ERR_INVALID, "next_obs must not be obs")
    big = torch.zeros((18, 128), dtype=torch.float32, device=DEV)
    refused(mlp, env._handle, {**a, "obs": big[:12], "next_obs": big[6:]}, KP1_ERR_INVALID, "must not overlap obs")
    refused(mlp, env._handle, {**a, "obs": big[6:], "terminal_obs": big[:12]}, KP1_ERR_INVALID, "must not overlap obs")
    assert not big.any()
    # an fp64 base env
    e64 = _single_env(cfgd, n, 128, real="f64")
    refused(mlp, e64._handle, a, KP1_ERR_UNSUPPORTED, "fp32 handle")
    e64.close()
    # a route longer than the LDS overlay
    from rl_brain_trainer_amd.ppo import ROUTE_FUSED_MAX_WAYPOINTS

    q = _route_q()
    W = ROUTE_FUSED_MAX_WAYPOINTS + 1
    x = np.linspace(0.0, q.shape[0] - 1.0, W)
    long_q = np.stack([np.interp(x, np.arange(q.shape[0]), q[:, k]) for k in range(7)], axis=1)
    elong = _single_env(cfgd, n, 128, route_q=long_q)
    refused(mlp, elong._handle, a, KP1_ERR_UNSUPPORTED, "KP1_ROUTE_FUSED_MAX_WAYPOINTS")
    elong.close()
    # anything but a route env: refused on the host
    arm = ArmKinematicVecEnv(kcfg.to_env_config(cfgd), n, seed=1)
    with pytest.raises(TypeError, match="RouteVecEnv"):
        mlp.forward_route_step(arm, a["obs"], **{k: v for k, v in a.items() if k != "obs"})
    arm.close()
    assert _untouched(a)
    # different devices: needs a second GPU; on a one-GPU machine say so in the test report
    if torch.cuda.device_count() > 1:
        m_other = MlpKernels(64, torch.device("cuda", 1), max_batch=128, obs_dim=80)
        refused(m_other, env._handle, a, KP1_ERR_INVALID, "different devices")
        m_other.close()
    else:
        warnings.warn("kp1_mlp_forward_route_step's different-devices refusal was not exercised: this machine has one GPU")
    # and the same arguments are accepted once nothing stands in the way (the chain is closed, the components are off)
    rc, msg = _raw_call(mlp, env._handle, **a)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert not _untouched(a)
    mlp.close()
    env.close()
