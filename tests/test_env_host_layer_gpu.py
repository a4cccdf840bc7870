"""Corners of the env handle's host layer that no other test reaches, at the grid-rounding edges of its one launcher:
N = 1 (one lane), 64 (one full 64-thread workgroup) and 65 (one workgroup plus one lane).

- ``kp1_get_state`` with some output pointers NULL: the arrays that are asked for are bit for bit those of the call that asks for all five,
  which is compared with the fp64 oracle by the rules of tests/env_control.py (f64: within F64_TOL; f32: q the two-float pair, the rest the
  fp32 cast, poses within F32_POSE_TOL).
- ``kp1_route_rng_set`` / ``kp1_route_rng_get`` on a population route handle: the streams a fresh handle holds are ``kp1_rng_seed_state`` of
  ``seeds[k] + i``, and a set -> get round trip returns every word, the buffered 32-bit half included; the base env's streams do not move.
- ``kp1_route_seed`` and through it ``kp1_seed`` (no other GPU test re-seeds a handle): both streams of env i restart at
  ``kp1_rng_seed_state(seed + first_env_id + i)``.
- ``step`` and ``step_into`` of the four handle classes (one text in ``DeviceEnvHandle`` for both families): the
  same bits in the handle's own buffers and in caller-owned ones at the padded pitch, and the same random streams afterwards.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest

import env_control as ec
from conftest import GOLDEN, load_golden_config
from oracle import oracle as orc
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import route_config as rcfg

pytestmark = pytest.mark.gpu

SIZES = [1, 64, 65]
STATE_WIDTH = {"q": 7, "dq": 7, "prev_action": 7, "goal_q": 7, "goal_pose6": 6}


@pytest.mark.parametrize("real", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_get_state_with_null_outputs(n, real):
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    cfg = load_golden_config("approach_default")
    env = ArmKinematicVecEnv(cfg, n, seed=806, real=real)
    env.set_curriculum_stage(3)
    ora = orc.OracleVecEnv(cfg, n, seed0=806, stage=3)
    env.reset()
    ec.reset(ora)
    stats = ec.Stats()
    full = ec.compare_state(env, ora, real, stats, ctx=f"n={n} {real}")
    keys = tuple(STATE_WIDTH)
    for asked in (("q",), ("goal_pose6",), ("dq", "goal_q"), ("prev_action", "goal_pose6"), ("q", "dq", "prev_action", "goal_q"), ()):
        out = {k: np.full((n, STATE_WIDTH[k]), np.nan) for k in asked}
        native.check(env.L.kp1_get_state(env._handle, *[out[k].ctypes.data if k in out else None for k in keys]))
        for k in asked:
            assert np.array_equal(out[k], full[k]), (n, real, asked, k)
    stats.report(f"test_get_state_with_null_outputs[{n}-{real}]")
    env.close()


def _seed_words(seed: int) -> list[int]:
    st = kcfg.RngState()
    native.check(native.load().kp1_rng_seed_state(seed, C.byref(st)))
    return [st.state_hi, st.state_lo, st.inc_hi, st.inc_lo, st.has_uint32, st.uinteger]


def _route_parts():
    cfgd = json.loads((GOLDEN / "configs" / "route_curriculum_prefix120_routeobs_sequence2.json").read_text())
    return kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=40), rcfg.load_route_q(GOLDEN / "synthetic_route.json")


@pytest.mark.parametrize("real", ["f64", "f32"])
def test_route_seed_restarts_both_streams(real):
    """kp1_route_seed (reset(seed=) of the wrapper): the wrapper's stream and the base env's (kp1_seed) of env i restart at seed + first_env_id + i"""
    from rl_brain_trainer_amd.route_env import RouteVecEnv

    n = 65
    env = RouteVecEnv(*_route_parts(), n, seed=5, real=real)
    created = np.array([_seed_words(5 + i) for i in range(n)], dtype=np.uint64)
    assert np.array_equal(env.rng_state(), created) and np.array_equal(env.base.rng_state(), created)
    env.reset()                                                    # the sampled reset draws from the wrapper's stream
    assert not np.array_equal(env.rng_state(), created)
    env.seed(2**32 + 9, first_env_id=3)
    again = np.array([_seed_words(2**32 + 9 + 3 + i) for i in range(n)], dtype=np.uint64)
    assert np.array_equal(env.rng_state(), again) and np.array_equal(env.base.rng_state(), again)
    env.close()


@pytest.mark.parametrize("replicas,n_per_replica", [(1, 1), (2, 32), (5, 13)], ids=["n1", "n64", "n65"])
def test_route_population_rng_set_get(replicas, n_per_replica):
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv

    seeds = [11, 2**32 + 5, 40, 7, 900][:replicas]      # (a seed above 32 bits takes SeedSequence's two-word path)
    n = replicas * n_per_replica
    pop = RoutePopulationVecEnv(*_route_parts(), seeds, n_per_replica)
    assert pop.n_envs == n in SIZES
    seeded = np.array([_seed_words(seeds[i // n_per_replica] + i % n_per_replica) for i in range(n)], dtype=np.uint64)
    assert np.array_equal(pop.rng_state(), seeded)
    assert np.array_equal(pop.base.rng_state(), seeded)          # kp1_route_create_population seeds both streams of env i alike
    rng = np.random.default_rng(n)
    words = rng.integers(0, 2**64, size=(n, 6), dtype=np.uint64)
    words[:, 3] |= np.uint64(1)                                   # a PCG64 increment is odd
    words[:, 4] = rng.integers(0, 2, size=n)                      # has_uint32
    words[:, 5] &= np.uint64(0xFFFFFFFF)                          # the buffered 32-bit half
    pop.set_rng_state(words)
    assert np.array_equal(pop.rng_state(), words)
    assert np.array_equal(pop.base.rng_state(), seeded)
    pop.set_rng_state(seeded)
    assert np.array_equal(pop.rng_state(), seeded)
    pop.close()


def _make_handle(family: str, real: str):
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv, RouteVecEnv
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    if family == "arm":
        return ArmKinematicVecEnv(load_golden_config("approach_default"), 64, seed=806, real=real)
    if family == "arm_population":
        return ArmKinematicPopulationVecEnv(load_golden_config("approach_default"), [806, 2**32 + 5], 32)
    if family == "route":
        return RouteVecEnv(*_route_parts(), 64, seed=806, real=real)
    return RoutePopulationVecEnv(*_route_parts(), [806, 2**32 + 5], 32)


@pytest.mark.parametrize("family,real", [("arm", "f32"), ("arm", "f64"), ("arm_population", "f32"), ("route", "f32"), ("route_population", "f32")])
def test_step_and_step_into_are_the_same_step(family, real):
    """``step`` into the handle's own buffers and ``step_into`` caller-owned ones at the padded pitch (64; 128 for the 80-float route
    observation) are one text in DeviceEnvHandle over the family's step call: two handles made from the same seed and stepped three times
    with the same actions give the same bits and leave the same random streams"""
    import torch

    own, into = _make_handle(family, real), _make_handle(family, real)
    n, width = own.n_envs, getattr(own, "obs_dim", kcfg.OBS_DIM)
    pitch = 64 if width <= 64 else 128
    assert n == 64 and width == (80 if family.startswith("route") else 56)
    own.set_obs_stride(pitch)
    into.set_obs_stride(pitch)
    assert torch.equal(own.reset(), into.reset())
    obs, term = (torch.zeros((n, pitch), dtype=torch.float32, device=own.device) for _ in range(2))
    reward, done = torch.zeros(n, dtype=own.dtype, device=own.device), torch.zeros(n, dtype=torch.uint8, device=own.device)
    gen = torch.Generator().manual_seed(45)
    for t in range(3):
        actions = (torch.rand((n, kcfg.NJ), generator=gen, dtype=torch.float64) * 2 - 1).to(device=own.device, dtype=own.dtype)
        got = own.step(actions)
        assert got[0] is own.obs and got[1] is own.reward and got[2] is own.done
        into.step_into(actions, obs, reward, done, term)
        for name, a, b in (("obs", own.obs, obs), ("reward", own.reward, reward), ("done", own.done, done), ("terminal_obs", own.terminal_obs, term)):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (family, real, t, name)
    assert np.array_equal(own.rng_state(), into.rng_state())
    if family.startswith("route"):
        assert np.array_equal(own.base.rng_state(), into.base.rng_state())
    own.close()
    into.close()
