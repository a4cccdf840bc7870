"""Record a teacher policy's (observation, action) pairs along the route for the teacher-anchor side loss.

Mirror of ``kinematic_phase1/route/collect_route_teacher_rollout.py`` (same arguments, same ``teacher_route_anchor_dataset.npz`` /
``teacher_route_anchor_summary.json``): the checkpoint is rolled deterministically through the sequential evaluation of the waypoints
``start_index .. end_index`` -- every episode starts from the final state of the previous one -- and stops at the first waypoint that does not
succeed; the samples of that waypoint are dropped.  Here the rollout is one device chain with ``stop_on_failure`` (route_env.RouteChain): per
step one policy forward and one kp1_route_chain_step, observations and actions written slice by slice into ``[S + 1, R, pitch]`` /
``[S, R, 7]`` blocks like the PPO rollout buffers, and a ``[S, R, 2]`` tag table naming the (route_index, step) of every sample.

    python -m rl_brain_trainer_amd.collect_route_teacher --checkpoint model.zip --config <route yaml> --route-path <route_q_dense.json> \
        --artifact-root /tmp/teacher --start-index 1 --end-index 120

``teacher_anchor.load_anchor_dataset`` reads the file back.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Any

import numpy as np

from . import config as kcfg
from . import route_config as rcfg

BLOCK_STEPS = 256     # lock steps recorded on the device between two copies to the host


def unflatten_observation(flat: np.ndarray, obs_dim: int) -> dict[str, np.ndarray]:
    """flat policy rows [M, >= obs_dim] -> the Dict observation's arrays, key -> [M, width]: the inverse of
    teacher_anchor.flatten_observation's layout table"""
    layout = rcfg.ROUTE_OBS_LAYOUT if obs_dim == rcfg.ROUTE_OBS_DIM else kcfg.OBS_LAYOUT
    flat = np.asarray(flat, dtype=np.float32)
    return {key: np.ascontiguousarray(flat[:, off:off + width]) for key, (off, width) in layout.items()}


def anchor_dataset_arrays(tags: np.ndarray, obs: np.ndarray, actions: np.ndarray, successful: list[set[int]], obs_dim: int) -> dict[str, np.ndarray]:
    """tags [T, R, 2] int32 (route_index, step; -1 once a row's chain has ended), obs [T, R, >= obs_dim], actions [T, R, 7] and, per row, the
    waypoints that succeeded -> the arrays of teacher_route_anchor_dataset.npz.  Samples of a waypoint that did not succeed are dropped; rows
    are kept one after another, each in time order."""
    tags = np.asarray(tags, dtype=np.int32)
    T, R = tags.shape[:2]
    picks_t, picks_r = [], []
    for r in range(R):
        ok = np.isin(tags[:, r, 0], np.fromiter(successful[r], dtype=np.int32, count=len(successful[r]))) & (tags[:, r, 0] >= 0)
        t = np.flatnonzero(ok)
        picks_t.append(t)
        picks_r.append(np.full(t.shape, r, dtype=np.int64))
    t_all = np.concatenate(picks_t) if picks_t else np.zeros(0, dtype=np.int64)
    r_all = np.concatenate(picks_r) if picks_r else np.zeros(0, dtype=np.int64)
    arrays: dict[str, np.ndarray] = {
        "actions": np.asarray(actions, dtype=np.float32)[t_all, r_all].reshape(-1, kcfg.NJ),
        "route_index": tags[t_all, r_all, 0].astype(np.int32),
        "step": tags[t_all, r_all, 1].astype(np.int32),
    }
    obs = np.asarray(obs, dtype=np.float32)
    flat = obs[t_all, r_all].reshape(len(t_all), obs.shape[-1])
    for key, value in unflatten_observation(flat, obs_dim).items():
        arrays[f"obs__{key}"] = value
    return arrays


def collect_teacher_rollout(*, checkpoint_path: Path, config_path: Path, route_path: Path, artifact_root: Path, start_index: int = 1,
                            end_index: int = 120, device: int = 0, block_steps: int = BLOCK_STEPS, one_launch: bool = False) -> dict[str, Any]:
    import torch

    from .ppo import InferencePolicy
    from .route_curriculum import check_chain_request
    from .route_env import RouteVecEnv
    from .train_route import load_route_training_config

    cfg = load_route_training_config(config_path)
    route_q = rcfg.load_route_q(route_path)
    W = int(route_q.shape[0])
    start, end = check_chain_request(replicas=1, n_waypoints=W, start_index=int(start_index), end_indices=[int(end_index)], rows_per_replica=1)
    policy = InferencePolicy.load(str(checkpoint_path), device=device)     # any width the MFMA kernels run, 2x256 included
    seq_off = {**cfg, "route": {**(cfg.get("route", {}) or {}), "sequence": {**((cfg.get("route", {}) or {}).get("sequence", {}) or {}), "enabled": False}}}
    base = kcfg.to_env_config(cfg)
    env = RouteVecEnv(base, rcfg.route_config_from_dict(seq_off, max_route_index=int(end_index)), route_q, 1, device=device, seed=0, real="f32")
    if env.obs_dim != policy.obs_dim:
        env.close()
        raise ValueError(f"the checkpoint reads {policy.obs_dim}-float observations, the route config produces {env.obs_dim}")
    chain = None
    try:
        mlp = policy._mlp
        pitch, R, S = int(mlp.obs_pad), 1, max(int(block_steps), 1)
        env.use_current_stream()
        env.set_obs_stride(pitch)
        dev = env.device
        obs_buf = torch.zeros((S + 1, R, pitch), dtype=torch.float32, device=dev)
        act_buf = torch.zeros((S, R, kcfg.NJ), dtype=torch.float32, device=dev)
        tag_buf = torch.full((S, R, 2), -1, dtype=torch.int32, device=dev)
        reward = torch.zeros(R, dtype=torch.float32, device=dev)
        done = torch.zeros(R, dtype=torch.uint8, device=dev)
        chain = env.chain(start, end, stop_on_failure=True)
        chain.begin(obs_buf[0])
        bound = (int(end[0]) - int(start[0]) + 1) * max(int(base.c.termination.max_episode_steps), 1)
        tags, obs_rows, act_rows = [], [], []
        taken = 0
        while taken < bound:
            n = min(S, bound - taken)
            for s in range(n):      # step s reads slice s and writes slice s + 1
                if one_launch:
                    chain.forward_step(mlp, obs_buf[s], obs_buf[s + 1], reward, done, action=act_buf[s], tags=tag_buf[s])
                else:
                    mlp.forward(obs_buf[s], clipped=act_buf[s])
                    chain.step(act_buf[s], obs_buf[s + 1], reward, done, tag_buf[s])
            taken += n
            tags.append(tag_buf[:n].cpu().numpy())
            obs_rows.append(obs_buf[:n].cpu().numpy())
            act_rows.append(act_buf[:n].cpu().numpy())
            if chain.alive() == 0:
                break
            obs_buf[0].copy_(obs_buf[n])
        records = chain.records()
    finally:
        if chain is not None:
            chain.close()
        env.close()
    successful = [{int(rec["route_index"]) for rec in row if rec["success"]} for row in records]
    failed = sorted(int(rec["route_index"]) for row in records for rec in row if not rec["success"])
    arrays = anchor_dataset_arrays(np.concatenate(tags), np.concatenate(obs_rows), np.concatenate(act_rows), successful, policy.obs_dim)
    artifact_root = Path(artifact_root)
    artifact_root.mkdir(parents=True, exist_ok=True)
    dataset_path = artifact_root / "teacher_route_anchor_dataset.npz"
    np.savez_compressed(dataset_path, **arrays)
    summary = {
        "schema_version": "v5.route_teacher_anchor_dataset.v1", "checkpoint": str(checkpoint_path), "config": str(config_path),
        "route_path": str(route_path), "dataset_path": str(dataset_path), "start_index": int(start_index), "requested_end_index": int(end_index),
        "successful_indices": sorted(i for s in successful for i in s), "failed_indices": failed, "sample_count": int(len(arrays["actions"])),
        "obs_keys": sorted(k[len("obs__"):] for k in arrays if k.startswith("obs__")),
        "action_dim": int(arrays["actions"].shape[1]) if len(arrays["actions"]) else 0,
    }
    (artifact_root / "teacher_route_anchor_summary.json").write_text(json.dumps(summary, indent=2))
    print(json.dumps(summary, indent=2))
    return summary


def build_arg_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Collect route teacher anchor dataset (MI355X engine).")
    p.add_argument("--checkpoint", required=True)
    p.add_argument("--config", required=True)
    p.add_argument("--route-path", required=True)
    p.add_argument("--artifact-root", required=True)
    p.add_argument("--start-index", type=int, default=1)
    p.add_argument("--end-index", type=int, default=120)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--one-launch", action="store_true", help="forward, step and hand-over of every lock step in ONE launch "
                   "(RouteChain.forward_step; hidden 64 / 128); the files are byte-equal to the default's")
    return p


def main(argv: list[str] | None = None) -> dict[str, Any]:
    args = build_arg_parser().parse_args(argv)
    return collect_teacher_rollout(checkpoint_path=Path(args.checkpoint), config_path=Path(args.config), route_path=Path(args.route_path),
                                   artifact_root=Path(args.artifact_root), start_index=args.start_index, end_index=args.end_index, device=args.device,
                                   one_launch=args.one_launch)


if __name__ == "__main__":
    main()
