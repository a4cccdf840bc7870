"""Shared by test_eval_step_h256_gpu.py, test_population_eval_gpu.py and test_eval_episodes_gpu.py: the constants, inputs and comparisons that
are the same in two or more of them.  The accumulators are evaluate.EpisodeBuffers, the form the runners use.  What differs per file (its
golden configs, its reset options, the population file's raw active mask, each file's refusal probe) stays in the file."""
from __future__ import annotations

import ctypes as C
import types

import numpy as np
import torch

from rl_brain_trainer_amd import evaluate as ev
from rl_brain_trainer_amd import ppo as P
from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

DEV = torch.device("cuda", 0)
THR = (0.30, 1.0, 2.0, 0.0)        # ready predicate of the step tests: pos, ori, |action| (exercises the norm), dq clause skipped
READY = types.SimpleNamespace(dock_coarse_ready_pos_threshold_m=THR[0], dock_coarse_ready_ori_threshold_rad=THR[1],
                              dock_coarse_ready_action_threshold=THR[2], dock_coarse_ready_dq_threshold=THR[3])
# Action-norm tensors, one-launch against the launch sequence: two orders of a 7-term fp64 sum plus a square root differ by a few ulp per
# step, summed over at most ~200 steps: about 2e-14 relative; 1e-13 is the bound
NORM_RTOL = 1e-13
NORM_KEYS = ("final_action_magnitude", "sum_action", "mean_action_magnitude")
ACTION_FLOATS = ("final_action_magnitude", "mean_final_action_magnitude")
NAMES = ev.EpisodeBuffers.NAMES


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def snapshot(b: ev.EpisodeBuffers) -> dict[str, torch.Tensor]:
    return {k: getattr(b, k).clone() for k in NAMES}


def state_dict(hidden: int, seed: int, obs_dim: int = 56, scale: float = 250.0) -> dict[str, torch.Tensor]:
    pol = P.ActorCritic(hidden, DEV, seed=seed, obs_dim=obs_dim)
    pol.views["action_net.weight"].mul_(scale)       # SB3's action head starts at gain 0.01: means of ~0.01 would never meet the clamp
    pol.views["action_net.bias"].copy_(torch.linspace(-0.3, 0.3, 7, device=DEV))
    return pol.state_dict()


def build_suite(cfg, episodes_per_stage: int) -> dict[str, np.ndarray]:
    """explicit resets: ``episodes_per_stage`` episodes each of stages 1 and 4 of ``cfg``'s curriculum-local suite"""
    parts = [ev.build_curriculum_local_eval_suite(cfg, seed=700001 + 1009 * s, stage_index=s, n_episodes=episodes_per_stage) for s in (1, 4)]
    return {k: np.concatenate([p[k] for p in parts]) for k in ("initial_q", "goal_q", "goal_pose6")}


def make_env(cfg, n: int, stride: int, opts: dict, **kw) -> ArmKinematicVecEnv:
    env = ArmKinematicVecEnv(cfg, n, seed=3, **kw)
    if stride != 56:
        env.set_obs_stride(stride)
    env.use_current_stream()
    env.reset(options=opts)
    return env


def forced_active_mask(n: int) -> torch.Tensor:
    """partly zero wherever there is more than one row"""
    m = np.random.default_rng(2).random(n) < 0.85
    m[0] = True
    if n > 1:
        m[1] = False
    return torch.tensor(m, device=DEV).to(torch.uint8).contiguous()


def norm_in_index_order(action: torch.Tensor) -> torch.Tensor:
    a = action.double()
    s = a[:, 0] * a[:, 0]
    for k in range(1, 7):
        s = s + a[:, k] * a[:, k]
    return s.sqrt().contiguous()


def assert_results_match(res, ref, what: str) -> None:
    assert set(res) == set(ref), what
    for k in ref:
        assert res[k].dtype == ref[k].dtype and res[k].shape == ref[k].shape, (what, k)
        if k in NORM_KEYS:
            rel = ((res[k] - ref[k]).abs() / ref[k].abs().clamp_min(1e-300)).max().item() if ref[k].numel() else 0.0
            print(f"{what} {k}: max relative difference {rel:.3e}, bit-equal {torch.equal(res[k], ref[k])}")
            assert torch.allclose(res[k], ref[k], rtol=NORM_RTOL, atol=0.0), (what, k, rel)
        else:
            assert torch.equal(res[k], ref[k]), (what, k)


def assert_payload_match(a, b, path="") -> None:
    """payloads equal; the action-magnitude floats to NORM_RTOL"""
    if isinstance(b, dict):
        assert isinstance(a, dict) and a.keys() == b.keys(), path
        for k in b:
            assert_payload_match(a[k], b[k], f"{path}/{k}")
    elif isinstance(b, list):
        assert isinstance(a, list) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            assert_payload_match(x, y, f"{path}[{i}]")
    elif isinstance(b, float) and path.rsplit("/", 1)[-1] in ACTION_FLOATS:
        assert abs(a - b) <= NORM_RTOL * abs(b), (path, a, b)
    else:
        assert a == b and type(a) is type(b), (path, a, b)


def trained_ppo(cfg):
    """a 2x256 PPO with graphs on after one iteration on 256 envs of ``cfg`` at curriculum stage 3 -> (ppo, env)"""
    env = ArmKinematicVecEnv(cfg, 256, seed=806)
    env.set_curriculum_stage(3)
    ppo = P.PPO(env, P.PPOConfig(n_steps=8, batch_size=1024, n_epochs=2, hidden=256, learning_rate=3e-3, seed=5), use_graphs=True)
    ppo.learn(256 * 8)
    return ppo, env
