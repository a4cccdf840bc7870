"""Finisher (dock-mode) trainer on one MI355X or one 8-GPU node.

Mirror of kinematic_phase1/training/train_dock_policy.py:39-131 (same YAML chain dock_default <- ppo_default <- overlay, same CLI
flags, same artefact names) on the device engine, plus the dock reverse curriculum the reference wires into its TD3 dock trainer
(train_dock_td3_policy.py:121-129: ``training.dock_reverse_curriculum``), running here as a device tracker inside the rollout graph.

    python -m rl_brain_trainer_amd.train_dock --config rl_brain_trainer_amd/configs/dock_workspace_handoff_noop_ft_12env.yaml \
        --run-id finisher --artifact-root /tmp/finisher --total-timesteps 2000000 --n-envs 4096
"""
from __future__ import annotations

import argparse
import functools
import json
from pathlib import Path
from typing import Any

from . import checkpoint
from . import config as kcfg
from .finisher_tools import DockReverseCurriculum
from .ppo import PPO, Dist, PPOConfig, run_training
from .trainer_cli import add_shared_flags, apply_switches, process_context, refuse_population_under_dp, replica_extra, write_json
from .vec_env import ArmKinematicVecEnv


def build_arg_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train the Phase 1B dock policy (MI355X engine).")
    p.add_argument("--config")
    p.add_argument("--run-id", default="dock_policy")
    p.add_argument("--artifact-root")
    p.add_argument("--total-timesteps", type=int)
    p.add_argument("--resume-from", help="a checkpoint zip; with --seeds also the artifact root of an earlier --seeds run (seed s resumes "
                                          "from seed_<s>/model_latest.zip)")
    p.add_argument("--n-envs", type=int, default=4096, help="environments per GPU")
    p.add_argument("--n-steps", type=int, default=64)
    p.add_argument("--batch-size", type=int, default=0, help="global minibatch; 0 = n_envs*n_steps*world/64")
    p.add_argument("--eval-episodes", type=int, default=512)
    g = p.add_mutually_exclusive_group()
    g.add_argument("--whole-episode-eval", dest="whole_episode_eval", action="store_const", const=True, default=None,
                   help="run the final dock evaluation with all its env steps in one launch (kp1_eval_episodes; implies --one-launch-eval); "
                        "same summary as --one-launch-eval")
    g.add_argument("--per-step-eval", dest="whole_episode_eval", action="store_const", const=False,
                   help="keep one launch per env step (kp1_eval_step) in that evaluation; without either flag it takes its "
                        "measured default (evaluate.WHOLE_EPISODES_DEFAULT), so the flag that names the default is a no-op")
    p.add_argument("--one-launch-eval", action="store_true",
                   help="run the final dock evaluation with the one-launch step (kp1_eval_step) instead of the launch sequence per env step "
                        "(evaluate.run_episodes, the default here: the one-launch form has not been timed on this workload); the summaries "
                        "are equal, the two forms differ only in the action-magnitude floats, by an ulp")
    add_shared_flags(p, artifact_flag="<artifact-root>")
    return p


def evaluate_dock(ppo: PPO, env_cfg: kcfg.EnvConfig, *, episodes: int, seed: int, device: int, one_launch: bool | None = None,
                  whole_episodes: bool | None = None) -> dict[str, Any]:
    """Deterministic dock evaluation on freshly sampled dock resets (eval_dock.py's summary keys that downstream scripts read).
    ``one_launch`` and ``whole_episodes`` as in evaluate.evaluate_workspace_expansion (None: the "evaluate_dock" row of
    evaluate.WHOLE_EPISODES_DEFAULT); either way the resets are drawn by env.reset(options=None) from the env's RNG."""
    from . import evaluate as ev

    env = ArmKinematicVecEnv(env_cfg, episodes, device=device, seed=seed)
    if ppo.obs_w != 56:
        env.set_obs_stride(ppo.obs_w)
    res, _ = ev.run_phase(env, ppo.predict, None, one_launch=one_launch, what="dock", whole_episodes=whole_episodes, entry="evaluate_dock")
    env.close()
    succ = res["success"].float()
    return {"episodes": int(episodes), "success_rate": float(succ.mean()), "mean_final_position_error": float(res["final_position_error"].mean()),
            "mean_final_orientation_error": float(res["final_orientation_error"].mean()), "mean_min_position_error": float(res["min_position_error"].mean()),
            "mean_episode_length": float(res["step_count"].float().mean())}


def status_line(ppo: PPO, it: int, steps: int, elapsed: float) -> str:
    """the --seed run's line at the logging cadence"""
    stage = ppo.curriculum.current_stage_index if ppo.curriculum is not None else -1
    return (f"[ppo-dock] it={it} steps={ppo.num_timesteps} fps={steps / elapsed:,.0f} stage={stage} "
            f"rew={ppo.rew_buf.mean().item():.4f} {ppo.last_stats}")


def main(argv: list[str] | None = None) -> dict[str, Any]:
    args = build_arg_parser().parse_args(argv)
    apply_switches(args)
    with process_context(args) as proc:
        return _main(args, proc)


def _main(args, proc) -> dict[str, Any]:
    world, rank, local_rank = proc.world, proc.rank, proc.device
    cfg = kcfg.load_dock_config(args.config)
    base_dirs = (Path(args.config).parent,) if args.config else ()
    env_cfg = kcfg.to_env_config(cfg, handoff_base_dirs=base_dirs)
    algo = kcfg.to_algorithm_kwargs(cfg, "ppo")
    runtime = cfg.get("training", {}) or {}
    if args.total_timesteps is not None:
        algo["total_timesteps"] = args.total_timesteps
    if args.seed is not None:
        algo["seed"] = args.seed
    seed = int(algo.get("seed", 0))
    root = Path(args.artifact_root) if args.artifact_root else kcfg.repo_root() / "artifacts/kinematic_phase1/phase1b_dock" / args.run_id
    if args.seeds is not None:
        return _main_population(args, cfg, env_cfg, algo, runtime, base_dirs, root, world, local_rank)
    if rank == 0:
        root.mkdir(parents=True, exist_ok=True)

    n_envs = args.n_envs
    from . import monitor as _monitor

    dist_glue = Dist()
    monitor = _monitor.cli_monitor(args)          # False, or the episode window
    _monitor.check_monitor(monitor, dist_glue)    # --monitor under data parallel: refused before any device work
    env = ArmKinematicVecEnv(env_cfg, n_envs, device=local_rank, seed=seed, first_env_id=rank * n_envs)
    batch = args.batch_size or max(n_envs * args.n_steps * world // 64, 64)
    model_kwargs = {k: v for k, v in algo.items() if k not in ("total_timesteps", "n_steps", "batch_size")}
    pcfg = PPOConfig.from_algo_kwargs(model_kwargs, n_steps=args.n_steps, batch_size=batch, hidden=checkpoint.hidden_for_run(args.hidden, args.resume_from))
    # training.dock_reverse_curriculum (train_dock_td3_policy.py:121-129): a device tracker after every env step, inside the rollout hipGraph
    curriculum = None
    cur_cfg = runtime.get("dock_reverse_curriculum", {}) or {}
    if bool(cur_cfg.get("enabled", False)):
        curriculum = DockReverseCurriculum(stages=list(cur_cfg.get("stages", [])), window_episodes=int(cur_cfg.get("window_episodes", 100)),
                                           handoff_base_dirs=base_dirs)
    ppo = proc.trainer = PPO(env, pcfg, curriculum=curriculum, dist=dist_glue, backend="hip", monitor=monitor)
    if args.resume_from and Path(args.resume_from).exists():
        # PPO.load(resume, env=vec_env) + learn(reset_num_timesteps=False) (train_dock_policy.py:89-102)
        ppo.load_checkpoint(args.resume_from, restore_timesteps=True, restore_hyperparameters=True)
        if rank == 0:
            print(f"Resuming dock policy from {args.resume_from}")

    wall, _ = run_training(ppo, int(algo.get("total_timesteps", 100_000)), log_every=args.log_every, status=status_line,
                           csv_paths=[root / "progress.csv"])
    if rank != 0:
        return {}
    summary = _final_artifacts(root, ppo, env_cfg, args=args, cfg=cfg, curriculum=curriculum, resume=args.resume_from, n_envs=n_envs * world,
                               world=world, seed=seed, device=local_rank, wall=wall)
    print(json.dumps(summary["dock_eval_summary"], indent=2))
    return summary


def _final_artifacts(root: Path, ppo, env_cfg: kcfg.EnvConfig, *, args, cfg: dict[str, Any], curriculum, resume, n_envs: int, world: int,
                     seed: int, device: int, wall: float, extra: dict[str, Any] | None = None) -> dict[str, Any]:
    """what a run leaves at its end: model_latest, the dock evaluation (dock_eval/) and training_summary.json (`ppo` is a PPO or a
    population replica)"""
    latest = root / "model_latest"
    checkpoint.save(latest, ppo, env_cfg)
    eval_summary = evaluate_dock(ppo, env_cfg, episodes=args.eval_episodes, seed=seed + 10_000, device=device,
                                 one_launch=None if getattr(args, "one_launch_eval", False) or getattr(args, "whole_episode_eval", None) else False,
                                 whole_episodes=getattr(args, "whole_episode_eval", None))
    write_json(root / "dock_eval" / "dock_eval_summary.json", eval_summary)
    summary = {"policy_type": "dock", "algorithm": "ppo", "run_id": args.run_id, "checkpoint_format": {"layout": "stable-baselines3 zip", "sb3_loadable": False, "finish_with": "tools/finish_sb3_zip.py (needs stable-baselines3==2.8.0)"}, "config": cfg, "model_path": str(latest) + ".zip",
               "resume_from": str(resume) if resume else None, "n_envs": n_envs, "device": f"{world}x MI355X",
               "dock_eval_summary": eval_summary, "dock_reverse_curriculum": curriculum.summary() if curriculum is not None else None,
               "num_timesteps": ppo.num_timesteps, "wall_seconds": wall, "env_steps_per_second": ppo.num_timesteps / wall, "update_form": ppo.update_form, **(extra or {})}
    write_json(root / "training_summary.json", summary)
    return summary


def _main_population(args, cfg, env_cfg, algo, runtime, base_dirs, root: Path, world: int, device: int) -> dict[str, Any]:
    """--seeds: the seeds train together as one DockPopulationPPO -- one env handle of K x n_envs envs and one tracker launch per env step for
    all seeds; seed s writes what a --seed s run writes, under root/seed_<s>/, plus population_summary.json.  Every seed is evaluated on its
    own config copy (its own reverse-curriculum stage).  --resume-from takes a checkpoint zip (every seed starts from it) or the root of an
    earlier --seeds run (seed s starts from seed_<s>/model_latest.zip).  The selection score of population_summary.json is each seed's dock
    evaluation success rate."""
    from .finisher_tools import DockReverseCurriculumPopulation
    from .population import DockPopulationPPO, plan_replicas, population_status, population_summary, resolve_resume_population
    from .vec_env import ArmKinematicPopulationVecEnv

    seeds, overrides, names = plan_replicas(args.seeds, args.sweep)
    refuse_population_under_dp(world)
    # refusals before any device work: the seeds, the width, and the checkpoints a population cannot resume together
    resume_paths = resolve_resume_population(args.resume_from, seeds, names)
    n_envs = args.n_envs
    batch = args.batch_size or max(n_envs * args.n_steps // 64, 64)
    model_kwargs = {k: v for k, v in algo.items() if k not in ("total_timesteps", "n_steps", "batch_size", "seed")}
    hidden = checkpoint.hidden_for_run(args.hidden, resume_paths[0] if resume_paths else None)
    pcfg = PPOConfig.from_algo_kwargs(model_kwargs, n_steps=args.n_steps, batch_size=batch, hidden=hidden)
    DockPopulationPPO._check_population_args(seeds, pcfg, None, None, overrides)
    cur_cfg = runtime.get("dock_reverse_curriculum", {}) or {}
    env = ArmKinematicPopulationVecEnv(env_cfg, seeds, n_envs, device=device, mode="dock", repeated_seeds=True)
    curriculum = None
    if bool(cur_cfg.get("enabled", False)):
        curriculum = DockReverseCurriculumPopulation(stages=list(cur_cfg.get("stages", [])), window_episodes=int(cur_cfg.get("window_episodes", 100)),
                                                     n_replicas=len(seeds), handoff_base_dirs=base_dirs)
    from . import monitor as _monitor

    pop = DockPopulationPPO(seeds, pcfg, env, curriculum=curriculum, overrides=overrides, monitor=_monitor.cli_monitor(args))
    if resume_paths is not None:
        pop.load_init_checkpoints(resume_paths)
        print(f"Resuming dock policies from {args.resume_from}")
    roots = [root / n for n in names]
    for r in roots:
        r.mkdir(parents=True, exist_ok=True)
    tag = "ppo-dock-population"
    wall, _ = run_training(pop, int(algo.get("total_timesteps", 100_000)), log_every=args.log_every,
                           status=functools.partial(population_status, tag=tag), csv_paths=[r / "progress.csv" for r in roots], tag=tag)
    rows = []
    for k, s in enumerate(seeds):
        rep = pop.replica(k)
        cur = curriculum.replica(k) if curriculum is not None else None
        cfg_k = cur.config if cur is not None else env_cfg
        resume = resume_paths[k] if resume_paths is not None else args.resume_from
        summ = _final_artifacts(roots[k], rep, cfg_k, args=args, cfg=cfg, curriculum=cur, resume=resume, n_envs=n_envs, world=1, seed=s,
                                device=device, wall=wall, extra=replica_extra(s, names[k], None if overrides is None else overrides[k]))
        rows.append({"seed": s, "artifact_root": str(roots[k]), "final_curriculum_stage": cur.current_stage_index if cur is not None else None,
                     "last_update_stats": rep.last_stats, "best_score": summ["dock_eval_summary"]["success_rate"], "model_latest": summ["model_path"]})
    summary = population_summary(pop, rows, wall_seconds=wall, selection="dock evaluation success_rate")
    write_json(root / "population_summary.json", summary)
    pop.close()
    if curriculum is not None:
        curriculum.close()
    env.close()
    return summary


if __name__ == "__main__":  # pragma: no cover
    main()
