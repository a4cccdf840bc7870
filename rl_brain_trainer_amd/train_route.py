"""Route-curriculum trainer on one or several MI355X (data parallel under torchrun, like train.py).

Mirror of ``kinematic_phase1/train_route_curriculum.py:69-199``: same YAML chain (approach_default <- ppo_default <- overlay), same
CLI flags, same artefacts (``model_latest.zip``, ``curriculum_history.json``, ``route_eval_sequential/``, ``route_gate/``,
``model_sequential_gate_accepted.zip``, ``training_summary.json``), with the reference's three callbacks mapped onto the device
engine: periodic checkpoints, the prefix curriculum (``RoutePrefixCurriculumDevice``: a one-wave tracker after every env step, inside the
rollout hipGraph) and the teacher-anchor imitation step between rollout and update (``RouteTeacherAnchor``).  The envs are ``RouteVecEnv`` lanes (single or
sequence wrapper, 56- or 80-float observation as the YAML says); the PPO update runs on the MFMA kernels.

    python -m rl_brain_trainer_amd.train_route --config <route yaml> --route-path <route_q_dense.json> --run-id route \
        --output-dir /tmp/route --total-timesteps 1000000 --n-envs 1024

Population: ``--seeds 7,8,9,10`` trains the seeds together on one GPU (RoutePopulationPPO: one route env handle and one tracker launch
per env step for all of them; 2x64 / 2x128 nets; with ``route.teacher_anchor.enabled`` every seed takes the anchor step on the same batch
through one launch sequence, PopulationTeacherAnchor).  Seed s writes under ``<output-dir>/seed_<s>/`` what a ``--seed s`` run writes, and
``population_summary.json`` names the best seed: gate accepted first, then the final sequential evaluation's longest success prefix, then
its success rate.

Data parallel: ``torchrun --nproc_per_node N -m rl_brain_trainer_amd.train_route ...`` (``--n-envs`` per rank, ``--batch-size`` the global
minibatch).  Rank r steps the envs r * n_envs .. (r + 1) * n_envs - 1 of the single-process run; the prefix curriculum replays every rank's
episode records in global env order (PPO._curriculum_observe), so all ranks promote together.  Rank 0 alone writes the artefacts and runs
the sequential evaluation and the gate.
"""
from __future__ import annotations

import argparse
import functools
import json
import shutil
import time
from pathlib import Path
from typing import Any

import torch

from . import checkpoint
from . import config as kcfg
from . import route_config as rcfg
from .ppo import PPO, Dist, PPOConfig, run_training
from .route_curriculum import (RoutePrefixCurriculumDevice, evaluate_route_gate, evaluate_sequential_route, evaluate_sequential_route_batch,
                               sliced_evaluate)
from .route_env import RouteVecEnv
from .teacher_anchor import PopulationTeacherAnchor, RouteTeacherAnchor, TeacherAnchorConfig
from .trainer_cli import add_shared_flags, apply_switches, process_context, refuse_population_under_dp, write_json


def load_route_training_config(path: str | Path | None) -> dict[str, Any]:
    """train_route_curriculum.py:41-45"""
    cfg = kcfg.deep_merge(kcfg.load_yaml_file(kcfg.builtin_config_dir() / "approach_default.yaml"), kcfg.load_yaml_file(kcfg.builtin_config_dir() / "ppo_default.yaml"))
    if path:
        cfg = kcfg.deep_merge(cfg, kcfg.load_yaml_file(Path(path)))
    return cfg


def build_arg_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train route curriculum policy (MI355X engine).")
    p.add_argument("--config", required=True)
    p.add_argument("--route-path")
    p.add_argument("--init-checkpoint")
    p.add_argument("--run-id", default="route_curriculum")
    p.add_argument("--output-dir")
    p.add_argument("--total-timesteps", type=int)
    p.add_argument("--n-envs", type=int, default=0, help="device environments (0 = training.n_envs of the YAML)")
    p.add_argument("--n-steps", type=int, default=0, help="rollout length (0 = the YAML's n_steps)")
    p.add_argument("--batch-size", type=int, default=0, help="minibatch (0 = the YAML's batch_size)")
    p.add_argument("--device", type=int, default=0, help="GPU of a single-process run (under torchrun: LOCAL_RANK)")
    p.add_argument("--one-launch-rollout", action="store_true", help="run every rollout step as ONE launch (kp1_mlp_forward_route_step: sets "
                   "KP1_FUSED_ROUTE_ROLLOUT=1; fp32, hidden 64 / 128, reward components off, not data parallel -- otherwise the launch "
                   "sequence stays); bit-identical to the default, for --seed and --seeds runs")
    p.add_argument("--per-replica-eval", action="store_true", help="with --seeds: run the final sequential evaluations and gates one replica and "
                   "one prefix after another on the host-driven evaluator, instead of one device chain per replica in lock step")
    p.add_argument("--chain-eval-form", choices=("launch-sequence", "one-launch-step", "whole-chain"), default=None, help="with --seeds: how the "
                   "chained final evaluation issues its lock steps -- the launch sequence, one launch per lock step "
                   "(kp1_mlp_forward_route_chain_step) or one launch per span of lock steps (kp1_route_chain_run); same files bit for bit. "
                   "Default: route_curriculum.CHAIN_FORM_DEFAULT.  --per-replica-eval and --seed keep their evaluators")
    add_shared_flags(p, artifact_flag="<output-dir>", log_every=0)
    return p


def _checkpoint_hook(checkpoint_freq: int, save):
    """PeriodicCheckpointCallback (callbacks.py) as run_training's ``after_update``: ``save(trainer, steps_taken)`` whenever the steps of
    this run pass the next multiple of ``checkpoint_freq``"""
    due = checkpoint_freq

    def after_update(trainer, steps: int) -> None:
        nonlocal due
        if steps >= due:
            save(trainer, steps)
            due += checkpoint_freq

    return after_update


def status_line(ppo: PPO, it: int, steps: int, elapsed: float, *, anchor=None) -> str:
    """the --seed run's line at the logging cadence"""
    s = ppo.curriculum.summary()
    return (f"[route] it={it} steps={ppo.num_timesteps} fps={steps / elapsed:,.0f} prefix={s['prefix_end_index']} "
            f"succ={s['recent_success_rate']:.3f} rew={ppo.rew_buf.mean().item():.4f} anchor={anchor.last_loss if anchor else 0.0:.5f}")


def population_status_line(pop, it: int, steps: int, elapsed: float) -> str:
    """the --seeds run's line at the logging cadence"""
    stages = [pop.pop_curriculum.summary(k)["prefix_end_index"] for k in range(pop.K)]
    anchor = pop.teacher_anchor
    return (f"[route-population] it={it} steps/replica={pop.num_timesteps} aggregate fps={pop.K * steps / elapsed:,.0f} prefixes={stages}"
            + (f" anchor={[round(v, 5) for v in anchor.last_loss]}" if anchor is not None else ""))


def main(argv: list[str] | None = None) -> dict[str, Any]:
    args = build_arg_parser().parse_args(argv)
    apply_switches(args)
    with process_context(args) as proc:     # WORLD_SIZE / RANK / LOCAL_RANK as torchrun sets them, or the caller's process group
        return _main(args, proc)


def _main(args, proc) -> dict[str, Any]:
    world, rank, device = proc.world, proc.rank, proc.device
    cfg = load_route_training_config(args.config)
    route_cfg = cfg.get("route", {}) or {}
    route_path = Path(args.route_path or route_cfg["route_path"])
    init_checkpoint = args.init_checkpoint or route_cfg.get("init_checkpoint")
    root = Path(args.output_dir) if args.output_dir else kcfg.repo_root() / "artifacts" / "kinematic_phase1" / "route_curriculum" / args.run_id
    if rank == 0:
        root.mkdir(parents=True, exist_ok=True)

    route_q = rcfg.load_route_q(route_path)
    W = int(route_q.shape[0])
    prefixes = rcfg.prefix_stages(cfg, W)
    env_cfg = kcfg.to_env_config(cfg)
    runtime_cfg = cfg.get("training", {}) or {}
    algo = kcfg.to_algorithm_kwargs(cfg, "ppo")
    if args.total_timesteps is not None:
        algo["total_timesteps"] = args.total_timesteps
    if args.seed is not None:
        algo["seed"] = args.seed
    seed = int(algo.get("seed") or 0)
    n_envs = int(args.n_envs or runtime_cfg.get("n_envs", 1))     # per rank
    if args.seeds is not None:
        return _main_population(args, cfg, route_cfg, route_path, route_q, prefixes, env_cfg, runtime_cfg, algo, init_checkpoint, root, n_envs,
                                world, device)
    from . import monitor as _monitor

    dist_glue = Dist()
    monitor = _monitor.cli_monitor(args)          # False, or the episode window
    _monitor.check_monitor(monitor, dist_glue)    # --monitor under data parallel: refused before any device work
    env = RouteVecEnv(env_cfg, rcfg.route_config_from_dict(cfg, max_route_index=prefixes[0]), route_q, n_envs, device=device, seed=seed,
                      first_env_id=rank * n_envs)

    total = int(algo.get("total_timesteps", 100_000))
    model_kwargs = {k: v for k, v in algo.items() if k not in ("total_timesteps", "n_steps", "batch_size")}
    n_steps = int(args.n_steps or algo.get("n_steps", 2048))
    batch = int(args.batch_size or algo.get("batch_size", 64))     # the global minibatch: PPO takes batch // world rows per rank
    pcfg = PPOConfig.from_algo_kwargs(model_kwargs, n_steps=n_steps, batch_size=batch, hidden=checkpoint.hidden_for_run(args.hidden, init_checkpoint))
    # the prefix curriculum: a device tracker after every env step (the rollout stays one hipGraph replay); data parallel: per-step episode
    # records, exchanged and replayed once per chunk of KP1_DONE_EXCHANGE_STEPS steps
    curriculum = RoutePrefixCurriculumDevice.from_config(cfg, W)
    ppo = proc.trainer = PPO(env, pcfg, curriculum=curriculum, dist=dist_glue, backend="hip", monitor=monitor)
    if init_checkpoint:
        # PPO.load(..., env=vec_env) + learn(reset_num_timesteps=False): weights, Adam state, step clock; the YAML's learning rate wins
        ppo.load_checkpoint(init_checkpoint, restore_timesteps=True, restore_hyperparameters=True)
        if rank == 0:
            print(f"Resuming route policy from {init_checkpoint}")

    anchor = None
    anchor_cfg = TeacherAnchorConfig(**(route_cfg.get("teacher_anchor", {}) or {}))
    if anchor_cfg.enabled:
        # every rank draws the same batch from the same default_rng(0) stream and steps identical parameters: the ranks stay in step
        anchor = RouteTeacherAnchor(anchor_cfg)
        anchor.on_training_start(ppo)

    def save_checkpoint(p, steps: int) -> None:
        if rank == 0:
            checkpoint.save(root / "checkpoints" / f"model_{steps}_steps", p, env_cfg)

    wall, steps = run_training(ppo, total, after_rollout=anchor.on_rollout_end if anchor is not None else None,     # (BaseCallback._on_rollout_end)
                               after_update=_checkpoint_hook(max(int(runtime_cfg.get("checkpoint_freq", 250_000)), 1), save_checkpoint),
                               log_every=args.log_every, status=functools.partial(status_line, anchor=anchor), csv_paths=[root / "progress.csv"])
    summary: dict[str, Any] = {}
    if rank == 0:     # the artefacts, the sequential evaluation and the gate
        rate = steps / max(wall, 1e-9)     # all ranks' env steps over the training loop
        summary = _write_run_artifacts(args, cfg, route_cfg, route_path, route_q, env_cfg, init_checkpoint, root, ppo, curriculum.summary(),
                                       anchor.summary() if anchor is not None else {"enabled": False}, n_envs * world, world, wall, rate, device)
    curriculum.close()
    env.close()
    return summary


# ------------------------------------------------------------------------------------------------------------------------ --seeds
POPULATION_SELECTION = ("route gate accepted first, then the longest_success_prefix of the final sequential evaluation, then its success_rate")


def _main_population(args, cfg: dict[str, Any], route_cfg: dict[str, Any], route_path: Path, route_q, prefixes: list[int], env_cfg, runtime_cfg,
                     algo: dict[str, Any], init_checkpoint, root: Path, n_envs: int, world: int, device: int) -> dict[str, Any]:
    """--seeds [--sweep]: the replicas train together as one RoutePopulationPPO; replica k writes what a --seed s_k run with its overrides
    writes under root/<replica name>/ (seed_<s> without --sweep)"""
    from .population import RoutePopulationPPO, plan_replicas, population_summary
    from .route_curriculum import RoutePrefixCurriculumPopulation
    from .route_env import RoutePopulationVecEnv

    seeds, overrides, names = plan_replicas(args.seeds, args.sweep)
    refuse_population_under_dp(world)
    hidden = checkpoint.hidden_for_run(args.hidden, init_checkpoint)
    if hidden not in (64, 128):
        raise ValueError(f"--seeds trains 2x64 / 2x128 nets: pass --hidden 64 or 128, or an --init-checkpoint of such a net (got a 2x{hidden} policy)")
    anchor = None
    anchor_cfg = TeacherAnchorConfig(**(route_cfg.get("teacher_anchor", {}) or {}))
    if anchor_cfg.enabled:
        # the dataset is opened and validated here, on the host, before any device work; every replica steps the same default_rng(0) batches
        anchor = PopulationTeacherAnchor(anchor_cfg)
    if init_checkpoint:
        RoutePopulationPPO.check_init_checkpoint(init_checkpoint)
    W = int(route_q.shape[0])
    total = int(algo.get("total_timesteps", 100_000))
    model_kwargs = {k: v for k, v in algo.items() if k not in ("total_timesteps", "n_steps", "batch_size")}
    n_steps = int(args.n_steps or algo.get("n_steps", 2048))
    batch = int(args.batch_size or algo.get("batch_size", 64))
    pcfg = PPOConfig.from_algo_kwargs(model_kwargs, n_steps=n_steps, batch_size=batch, hidden=hidden)
    RoutePopulationPPO._check_population_args(seeds, pcfg, None, None, overrides)     # refusals before any device work
    roots = [root / n for n in names]
    for r in roots:
        r.mkdir(parents=True, exist_ok=True)
    env = RoutePopulationVecEnv(env_cfg, rcfg.route_config_from_dict(cfg, max_route_index=prefixes[0]), route_q, seeds, n_envs, device=device)
    curriculum = RoutePrefixCurriculumPopulation.from_config(cfg, W)
    pop = None
    try:
        from . import monitor as _monitor

        pop = RoutePopulationPPO(seeds, pcfg, env, curriculum=curriculum, overrides=overrides, teacher_anchor=anchor, monitor=_monitor.cli_monitor(args))
        if init_checkpoint:
            pop.load_init_checkpoint(init_checkpoint)
            print(f"Resuming every route policy of the population from {init_checkpoint}")

        def save_checkpoints(p, steps: int) -> None:
            for k in range(p.K):
                checkpoint.save(roots[k] / "checkpoints" / f"model_{steps}_steps", p.replica(k), env_cfg)

        # (the anchor steps after the rollout, before the update, as in the --seed loop)
        wall, steps = run_training(pop, total, after_rollout=anchor.on_rollout_end if anchor is not None else None,
                                   after_update=_checkpoint_hook(max(int(runtime_cfg.get("checkpoint_freq", 250_000)), 1), save_checkpoints),
                                   log_every=args.log_every, status=population_status_line, csv_paths=[r / "progress.csv" for r in roots],
                                   tag="route-population")
        rate = steps / max(wall, 1e-9)     # env steps of one replica per second of the population's training loop
        rows = []
        curriculum_summaries = [curriculum.summary(k) for k in range(pop.K)]
        evaluators: list[Any] = [None] * pop.K
        batch_share = 0.0
        if not args.per_replica_eval:
            # ONE chain per replica to the largest index any of its evaluations asks for; every evaluation of the replica (the reached prefix,
            # the gate's prefixes, the full route) is then a slice of that chain's rows
            t_batch = time.time()
            ends = [_chain_end_index(route_cfg, cs, W) for cs in curriculum_summaries]
            chains = evaluate_sequential_route_batch(mlp=pop._mlp, cfg=cfg, route_q=route_q, start_index=1, end_indices=ends, device=device,
                                                     form=args.chain_eval_form.replace("-", "_") if args.chain_eval_form else None)
            evaluators = [sliced_evaluate(c["rows"], c["final_qs"], env.route_progress_m) for c in chains]
            batch_share = (time.time() - t_batch) / pop.K
        for k, s in enumerate(seeds):   # the artefacts and the gate verdicts are written one seed after another, as single runs write them
            summary = _write_run_artifacts(args, cfg, route_cfg, route_path, route_q, env_cfg, init_checkpoint, roots[k], pop.replica(k),
                                           curriculum_summaries[k], anchor.summary() if anchor is not None else {"enabled": False}, n_envs, 1, wall,
                                           rate, device, evaluate=evaluators[k],
                                           evaluation_wall_offset=batch_share)
            ev, gate = summary["route_eval_sequential_summary"], summary["route_gate_summary"]
            accepted = bool(gate.get("accepted", False))
            score = [int(accepted), int(ev.get("longest_success_prefix", 0) or 0), float(ev.get("success_rate", 0.0) or 0.0)]
            rows.append({"seed": s, "prefix_end_index": summary["curriculum_summary"]["prefix_end_index"], "gate_accepted": accepted,
                         "longest_success_prefix": score[1], "success_rate": score[2], "best_score": score,
                         "model_path": str(roots[k] / "model_latest.zip"), "evaluation_wall_seconds": summary["evaluation_wall_seconds"],
                         "last_stats": pop.replica_stats(k)})
        out = population_summary(pop, rows, wall_seconds=wall, selection=POPULATION_SELECTION)
        out["aggregate_env_steps_per_second"] = pop.K * rate     # the steps of this run, not the init checkpoint's clock
        out["teacher_anchor_steps"] = int(pop.actor_extra_steps)   # anchor steps every replica's actor tensors took on top of the common count
        write_json(root / "population_summary.json", out, default=str)
        print(json.dumps({"run_id": args.run_id, "artifact_root": str(root), "seeds": seeds, "best_seed": out["best_seed"],
                          "aggregate_env_steps_per_second": out["aggregate_env_steps_per_second"]}, indent=2))
        return out
    finally:
        if pop is not None:
            pop.close()
        curriculum.close()
        env.close()


def _gate_config(route_cfg: dict[str, Any]) -> dict[str, Any]:
    return route_cfg.get("sequential_gate", {}) or {}


def _chain_end_index(route_cfg: dict[str, Any], curriculum_summary: dict[str, Any], n_waypoints: int) -> int:
    """the largest end index _write_run_artifacts evaluates for one replica: the reached prefix and, with the gate on, its prefixes and the
    full route (every index clamped to the route as evaluate_sequential_route clamps it)"""
    last = n_waypoints - 1
    ends = [min(int(curriculum_summary["prefix_end_index"]), last)]
    gate_cfg = _gate_config(route_cfg)
    if bool(gate_cfg.get("enabled", False)):
        ends += [min(int(x) or last, last) for x in gate_cfg.get("prefixes", [20, 40, 80, 120, 180])]
        if gate_cfg.get("full_end_index") is not None:
            ends.append(min(int(gate_cfg["full_end_index"]) or last, last))
    return max(ends)


def _write_run_artifacts(args, cfg: dict[str, Any], route_cfg: dict[str, Any], route_path: Path, route_q, env_cfg, init_checkpoint, root: Path, ppo,
                         curriculum_summary: dict[str, Any], anchor_summary: dict[str, Any], n_envs_total: int, world: int, wall: float, rate: float,
                         device: int, evaluate=None, evaluation_wall_offset: float = 0.0) -> dict[str, Any]:
    """What a run leaves under `root` once training ends: model_latest.zip, curriculum_history.json, the sequential evaluation of the
    reached prefix, the gate (and model_sequential_gate_accepted.zip) and training_summary.json.  `ppo` is a PPO or a population replica.
    ``evaluate``: a ready ``evaluate(artifact_root=, start_index=, end_index=)`` (the population's sliced chain) in place of the host-driven
    evaluator on ``ppo.predict``; ``evaluation_wall_offset``: this replica's share of the wall time that callable's chain took."""
    W = int(route_q.shape[0])
    latest = root / "model_latest"
    checkpoint.save(latest, ppo, env_cfg)
    write_json(root / "curriculum_history.json", curriculum_summary)

    def policy(obs: torch.Tensor) -> torch.Tensor:
        return ppo.predict(obs.float().contiguous(), deterministic=True)

    def evaluate_on_host(*, artifact_root: Path, start_index: int, end_index: int) -> dict[str, Any]:
        out = evaluate_sequential_route(policy=policy, cfg=cfg, route_q=route_q, artifact_root=artifact_root, start_index=start_index, end_index=end_index,
                                        device=device)
        return {k: v for k, v in out.items() if k not in ("rows", "chunk_metrics", "final_q")}

    evaluate = evaluate or evaluate_on_host

    eval_end = min(int(curriculum_summary["prefix_end_index"]), W - 1)
    t_eval = time.time()
    eval_summary = evaluate(artifact_root=root / "route_eval_sequential", start_index=1, end_index=eval_end)
    gate_summary: dict[str, Any] = {"enabled": False}
    gate_cfg = _gate_config(route_cfg)
    if bool(gate_cfg.get("enabled", False)):
        gate_summary = evaluate_route_gate(evaluate=evaluate, artifact_root=root / "route_gate", prefixes=[int(x) for x in gate_cfg.get("prefixes", [20, 40, 80, 120, 180])],
                                           full_end_index=gate_cfg.get("full_end_index"),
                                           min_prefix120_success_rate=float(gate_cfg.get("min_prefix120_success_rate", 0.98)),
                                           best_full_longest_prefix=int(gate_cfg.get("best_full_longest_prefix", 170)),
                                           full_prefix_tolerance=int(gate_cfg.get("full_prefix_tolerance", 20)), checkpoint=str(latest), config=str(args.config),
                                           route_path=str(route_path))
        if bool(gate_summary.get("accepted", False)):
            src = Path(str(latest) + ".zip")
            dst = root / "model_sequential_gate_accepted.zip"
            if src.exists():
                shutil.copy2(src, dst)
                gate_summary["accepted_model_path"] = str(dst)
    summary = {
        "schema_version": "v5.route_curriculum.training_summary.v1", "run_id": args.run_id, "route_path": str(route_path),
        "init_checkpoint": str(init_checkpoint) if init_checkpoint else None, "checkpoint_format": {"layout": "stable-baselines3 zip", "sb3_loadable": False, "finish_with": "tools/finish_sb3_zip.py (needs stable-baselines3==2.8.0)"}, "model_path": str(latest), "n_envs": n_envs_total, "device": "MI355X" if world == 1 else f"{world}x MI355X",
        "world_size": world,
        "curriculum_summary": curriculum_summary, "teacher_anchor_summary": anchor_summary,
        "route_eval_sequential_summary": eval_summary, "route_gate_summary": gate_summary, "config": cfg,
        "num_timesteps": int(ppo.num_timesteps), "wall_seconds": wall, "env_steps_per_second": rate, "env_steps_per_s": rate,
        "observation_dim": int(ppo.obs_dim), "update_form": ppo.update_form,
    }
    # the sequential evaluation and the gate, after training (a population's chained evaluation: its share of the one batch call + its own files)
    summary["evaluation_wall_seconds"] = time.time() - t_eval + evaluation_wall_offset
    write_json(root / "training_summary.json", summary, default=str)
    print(json.dumps({"run_id": args.run_id, "artifact_root": str(root), "model_latest": str(latest) + ".zip", "prefix_end_index": curriculum_summary["prefix_end_index"],
                      "env_steps_per_second": summary["env_steps_per_second"]}, indent=2))
    return summary


if __name__ == "__main__":
    main()
