#!/usr/bin/env python3
"""What the training monitor adds to a PPO iteration at the benchmark's shape (developer tool, not bench.py).

bench.py's headline workload -- workspace_expansion_bigtrain.yaml, stage 5, 4096 envs x 128 steps, minibatch 8192, 8 epochs, 2x256, graphs
on -- built twice in one process, once with ``monitor=False`` and once with ``monitor=True``, and timed alternately: ``--repeats`` blocks
of ``--steps`` iterations each per form, device-synchronised at both ends of a block.  Reports the median and the max - min of the
per-iteration time of each form and their difference, and the monitor's record of the last iteration.

    python tools/monitor_bench.py [--steps 8] [--repeats 3] [--out profiles/episode_monitor_bench_shape.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from rl_brain_trainer_amd import config as kcfg  # noqa: E402
from rl_brain_trainer_amd.curriculum import PointCurriculum  # noqa: E402
from rl_brain_trainer_amd.ppo import PPO, PPOConfig  # noqa: E402
from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv  # noqa: E402


def build(args, monitor: bool) -> PPO:
    cfg_dict = kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml")
    env_cfg = kcfg.to_env_config(cfg_dict)
    algo = kcfg.to_algorithm_kwargs(cfg_dict)
    seed = int(algo["seed"])
    env = ArmKinematicVecEnv(env_cfg, args.envs, seed=seed)
    cur_cfg = cfg_dict["env"]["curriculum"]
    curriculum = PointCurriculum(success_rate_threshold=cur_cfg["success_rate_threshold"], window_episodes=cur_cfg["window_episodes"],
                                 min_episodes_per_stage=cur_cfg["min_episodes_per_stage"], max_stage_index=args.stage, initial_stage_index=args.stage)
    pcfg = PPOConfig(learning_rate=algo["learning_rate"], n_steps=args.n_steps, batch_size=args.batch, n_epochs=args.epochs, gamma=algo["gamma"],
                     gae_lambda=algo["gae_lambda"], clip_range=algo["clip_range"], ent_coef=algo["ent_coef"], seed=seed, hidden=args.hidden)
    return PPO(env, pcfg, curriculum=curriculum, monitor=monitor)


def block_ms(ppo: PPO, steps: int) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ppo.collect_rollouts()
        ppo.train()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=8, help="iterations per timed block")
    ap.add_argument("--repeats", type=int, default=3, help="timed blocks per form, alternating")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--stage", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    runs = {"monitor_off": build(args, False), "monitor_on": build(args, True)}
    for ppo in runs.values():
        block_ms(ppo, args.warmup)
    times: dict[str, list[float]] = {name: [] for name in runs}
    for _ in range(args.repeats):
        for name, ppo in runs.items():
            times[name].append(block_ms(ppo, args.steps))
    identical = bool(torch.equal(runs["monitor_off"].policy.flat, runs["monitor_on"].policy.flat))
    out = {"workload": f"bench.py headline shape: {args.envs} envs x {args.n_steps} steps, minibatch {args.batch}, {args.epochs} epochs, 2x{args.hidden}, "
                       f"stage {args.stage}, graphs on; {args.repeats} alternating blocks of {args.steps} iterations per form",
           "device": torch.cuda.get_device_name(0),
           **{name: {"iteration_ms_median": statistics.median(v), "iteration_ms_spread": max(v) - min(v), "iteration_ms_blocks": v} for name, v in times.items()},
           "added_ms_per_iteration": statistics.median(times["monitor_on"]) - statistics.median(times["monitor_off"]),
           "parameters_bit_identical_after_the_run": identical, "last_record": runs["monitor_on"].monitor_rows()[0]}
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=2) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
