"""Stage 0-11 Approach trainer on one MI355X or one 8-GPU node.

Mirror of the reference entry point kinematic_phase1/train_workspace_expansion.py:144-270 (same YAML chain, same CLI
flags, same artefact names) with the SubprocVecEnv + SB3 loop replaced by the device-resident engine:

    python -m rl_brain_trainer_amd.train --config rl_brain_trainer_amd/configs/workspace_expansion_bigtrain.yaml \
        --run-id demo --artifact-root /tmp/run --total-timesteps 2000000 --n-envs 4096
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m rl_brain_trainer_amd.train ...

Differences forced by scale, all explicit flags: ``--n-envs`` (per GPU, default 4096 instead of the YAML's 16),
``--n-steps`` / ``--batch-size`` (defaults keep the reference's 64 minibatches per epoch), ``--hidden`` (256, BASELINE
config 2; the reference never sets net_arch, i.e. SB3's 64).
"""
from __future__ import annotations

import argparse
import functools
import json
import shutil
from pathlib import Path
from typing import Any

from . import checkpoint
from . import config as kcfg
from .curriculum import PointCurriculum
from .ppo import PPO, Dist, PPOConfig, run_training, status_line
from .trainer_cli import add_shared_flags, apply_switches, process_context, refuse_population_under_dp, replica_extra, write_json
from .vec_env import ArmKinematicVecEnv


def build_arg_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Workspace Expansion Curriculum PPO training (MI355X engine).")
    p.add_argument("--config", required=True)
    p.add_argument("--run-id", default="workspace_expand_mi355x_001")
    p.add_argument("--artifact-root")
    p.add_argument("--total-timesteps", type=int)
    p.add_argument("--resume-from")
    p.add_argument("--no-gate-callback", action="store_true")
    p.add_argument("--per-replica-eval", action="store_true", help="with --seeds: evaluate the replicas one after another (K gate evaluations per gate "
                   "instant) instead of all of them in one population evaluation")
    p.add_argument("--n-envs", type=int, default=4096, help="environments per GPU")
    p.add_argument("--n-steps", type=int, default=128)
    p.add_argument("--batch-size", type=int, default=0, help="global minibatch; 0 = n_envs*n_steps*world/64")
    p.add_argument("--learning-rate", type=float)
    g = p.add_mutually_exclusive_group()
    g.add_argument("--whole-episode-eval", dest="whole_episode_eval", action="store_const", const=True, default=None,
                   help="run the gate and final evaluations with all env steps of a phase in one launch (kp1_eval_episodes) where the one-launch "
                        "step covers the phase; same results bit for bit")
    g.add_argument("--per-step-eval", dest="whole_episode_eval", action="store_const", const=False,
                   help="keep one launch per env step (kp1_eval_step) in those evaluations; without either flag every evaluation takes its "
                        "measured default (evaluate.WHOLE_EPISODES_DEFAULT), so the flag that names the default is a no-op")
    r = p.add_mutually_exclusive_group()
    r.add_argument("--whole-rollout", dest="whole_rollout", action="store_const", const=True, default=None,
                   help="run all env steps of a rollout in one launch per span (kp1_rollout_run; sets KP1_ROLLOUT_RUN=1) where it is covered: "
                        "hidden 64 / 128, one process, no tracker or at most 32 envs per seed; same results bit for bit")
    r.add_argument("--per-step-rollout", dest="whole_rollout", action="store_const", const=False,
                   help="keep one launch per env step (sets KP1_ROLLOUT_RUN=0); without either flag KP1_ROLLOUT_RUN decides, and unset it is "
                        "the trainer's default (the per-step loop)")
    p.add_argument("--multi-launch-eval", action="store_true",
                   help="with --seed: run the gate and final evaluations as the launch sequence per env step (evaluate.run_episodes) instead of "
                        "the one-launch step (kp1_eval_step); the two forms agree bit for bit except in the action-magnitude floats "
                        "(final / mean action magnitude), which may differ by an ulp (and a ready bit, should a norm sit on its threshold to the last bit)")
    add_shared_flags(p, artifact_flag="<artifact-root>", sweep_under="<artifact-root>/", train_tile_group=r)
    return p


class WorkspaceEvalGate:
    """WorkspaceEvalGateCallback (train_workspace_expansion.py:54-129): every ``eval_interval`` timesteps save a candidate, run the
    deterministic Approach -> Finisher stage suites on it, append the gated selection to eval_history.jsonl and keep the best
    retention-ok candidate as best_checkpoint/model_best_by_gate.zip.  The reference checks after every env step of its 12-16
    envs; here the check runs after every PPO iteration (n_envs * n_steps timesteps), so evaluations land on iteration boundaries."""

    def __init__(self, *, artifact_root: Path, approach_cfg: kcfg.EnvConfig, finisher_policy, finisher_cfg: kcfg.EnvConfig | None, eval_interval: int,
                 episodes: int, seed: int, stage_indices: list[int], gate_config: dict[str, Any], device: int = 0, one_launch: bool | None = None,
                 whole_episodes: bool | None = None) -> None:
        self.artifact_root = artifact_root
        self.approach_cfg, self.finisher_policy, self.finisher_cfg = approach_cfg, finisher_policy, finisher_cfg
        self.eval_interval = max(int(eval_interval), 1)
        self.episodes = max(int(episodes), 1)
        self.seed = int(seed)
        self.stage_indices = list(stage_indices)
        self.gate_config = dict(gate_config)
        self.device = device
        self.one_launch = one_launch        # evaluate.evaluate_workspace_expansion's switch (None: the one-launch step where covered)
        self.whole_episodes = whole_episodes    # likewise (None: the entry point's measured default)
        self.candidates_dir = artifact_root / "gate_candidates"
        self.eval_dir = artifact_root / "gate_evals"
        self.best_dir = artifact_root / "best_checkpoint"
        self.eval_history_path = artifact_root / "eval_history.jsonl"
        for d in (self.candidates_dir, self.eval_dir, self.best_dir):
            d.mkdir(parents=True, exist_ok=True)
        self.best_score = float("-inf")
        self.next_eval_timesteps = self.eval_interval

    def due(self, num_timesteps: int) -> bool:
        """whether an evaluation falls at this step count (then the next one is scheduled)"""
        if num_timesteps < self.next_eval_timesteps:
            return False
        while self.next_eval_timesteps <= num_timesteps:
            self.next_eval_timesteps += self.eval_interval
        return True

    def save_candidate(self, ppo, env_cfg: kcfg.EnvConfig) -> Path:
        candidate = self.candidates_dir / f"candidate_step_{ppo.num_timesteps}"
        checkpoint.save(candidate, ppo, env_cfg)
        return candidate

    def eval_root(self, num_timesteps: int) -> Path:
        return self.eval_dir / f"eval_step_{num_timesteps}"

    def record(self, ppo, env_cfg: kcfg.EnvConfig, candidate: Path, summary: dict[str, Any]) -> dict[str, Any]:
        """an evaluation's selection -> eval_history.jsonl; a retention-ok best score -> best_checkpoint/model_best_by_gate.zip"""
        selection = summary["best_model_selection"]
        record = {"timesteps": int(ppo.num_timesteps), "candidate": str(candidate) + ".zip", **selection}
        with self.eval_history_path.open("a", encoding="utf-8") as handle:
            handle.write(json.dumps(record) + "\n")
        score = float(selection["score"])
        if bool(selection["retention_ok"]) and score > self.best_score:
            self.best_score = score
            checkpoint.save(self.best_dir / "model_best_by_gate", ppo, env_cfg)
            write_json(self.artifact_root / "best_model_selection_summary.json", record)
        return record

    def on_iteration(self, ppo: PPO, env_cfg: kcfg.EnvConfig) -> dict[str, Any] | None:
        from . import evaluate as ev

        if not self.due(ppo.num_timesteps):
            return None
        candidate = self.save_candidate(ppo, env_cfg)
        summary = ev.evaluate_workspace_expansion(approach_policy=ppo.predict, finisher_policy=self.finisher_policy, approach_cfg=self.approach_cfg,
                                                  finisher_cfg=self.finisher_cfg, episodes=self.episodes, seed=self.seed, stage_indices=self.stage_indices,
                                                  gate_config=self.gate_config, artifact_root=self.eval_root(ppo.num_timesteps),
                                                  device=self.device, obs_stride=ppo.obs_w, one_launch=self.one_launch,
                                                  whole_episodes=self.whole_episodes)
        return self.record(ppo, env_cfg, candidate, summary)


def population_gate_iteration(gates: dict[int, WorkspaceEvalGate], pop, env_cfg: kcfg.EnvConfig) -> list[dict[str, Any]] | None:
    """the gate instant of a population whose every replica has a gate (all on one clock): K candidates, ONE population evaluation
    (evaluate.evaluate_workspace_expansion_population: one launch per env step for all replicas), K history records"""
    from . import evaluate as ev

    due = [g.due(pop.num_timesteps) for g in gates.values()]
    if not any(due):
        return None
    assert all(due) and sorted(gates) == list(range(pop.K)), "the replicas' gates share one clock"
    g0 = gates[0]
    reps = [pop.replica(k) for k in range(pop.K)]
    candidates = [gates[k].save_candidate(reps[k], env_cfg) for k in range(pop.K)]
    payloads = ev.evaluate_workspace_expansion_population(population=pop, finisher_policy=g0.finisher_policy, approach_cfg=g0.approach_cfg,
                                                          finisher_cfg=g0.finisher_cfg, episodes=g0.episodes, seed=g0.seed, stage_indices=g0.stage_indices,
                                                          gate_config=g0.gate_config, artifact_roots=[gates[k].eval_root(pop.num_timesteps) for k in range(pop.K)],
                                                          device=g0.device, whole_episodes=g0.whole_episodes)
    return [gates[k].record(reps[k], env_cfg, candidates[k], payloads[k]) for k in range(pop.K)]


def main(argv: list[str] | None = None) -> dict[str, Any]:
    args = build_arg_parser().parse_args(argv)
    apply_switches(args)
    with process_context(args) as proc:
        return _main(args, proc)


def _main(args, proc) -> dict[str, Any]:
    world, rank, local_rank = proc.world, proc.rank, proc.device
    cfg = kcfg.load_workspace_expansion_config(args.config)
    # env.route_reset.route_path: absolute, under the working directory, or next to the config file
    env_cfg = kcfg.to_env_config(cfg, handoff_base_dirs=(Path(args.config).resolve().parent,) if args.config else ())
    algo = kcfg.to_algorithm_kwargs(cfg, "ppo")
    ws = cfg.get("workspace_expansion", {})
    if args.total_timesteps is not None:
        algo["total_timesteps"] = args.total_timesteps
    if args.seed is not None:
        algo["seed"] = args.seed
    if args.learning_rate is not None:
        algo["learning_rate"] = args.learning_rate
    seed = int(algo.get("seed", 0))

    root = Path(args.artifact_root) if args.artifact_root else kcfg.repo_root() / "artifacts/kinematic_phase1/workspace_expansion" / args.run_id
    n_envs = args.n_envs
    batch = args.batch_size or max(n_envs * args.n_steps * world // 64, 64)
    model_kwargs = {k: v for k, v in algo.items() if k not in ("total_timesteps", "n_steps", "batch_size", "seed")}
    resume = args.resume_from or ws.get("init_approach_checkpoint", "")
    if args.seeds is not None:
        return _main_population(args, cfg, env_cfg, algo, ws, root, batch, model_kwargs, resume, world, local_rank)
    hidden = checkpoint.hidden_for_run(args.hidden, resume)     # a reference-trained zip is 2x64: the model takes the checkpoint's width
    if rank == 0:
        _start_artifacts(root, args, cfg)

    from . import monitor as _monitor

    dist_glue = Dist()
    monitor = _monitor.cli_monitor(args)          # False, or the episode window
    _monitor.check_monitor(monitor, dist_glue)    # --monitor under data parallel: refused before any device work
    env = ArmKinematicVecEnv(env_cfg, n_envs, device=local_rank, seed=seed, first_env_id=rank * n_envs)
    curriculum = _make_curriculum(cfg, env_cfg, ws, local_rank)
    pcfg = PPOConfig.from_algo_kwargs(model_kwargs, n_steps=args.n_steps, batch_size=batch, hidden=hidden, seed=seed)
    ppo = proc.trainer = PPO(env, pcfg, curriculum=curriculum, dist=dist_glue, backend="hip", monitor=monitor)     # 2x64 / 2x128 / 2x256 all run on the MFMA kernels
    if resume and Path(resume).exists():
        # PPO.load(resume, env=vec_env): weights, Adam state and the saved algorithm constants; the YAML's learning rate is re-applied
        ppo.load_checkpoint(resume, restore_hyperparameters=True)
        if rank == 0:
            print(f"Resuming workspace expansion from {resume}")

    gate = None
    finisher_policy, finisher_cfg = _load_finisher(ws, local_rank)
    gate_cfg = dict(ws.get("gate", {}) or {})
    if rank == 0 and not args.no_gate_callback and finisher_policy is not None:
        gate = _make_gate(root, env_cfg, finisher_policy, finisher_cfg, ws, gate_cfg, local_rank, one_launch=False if args.multi_launch_eval else None,
                          whole_episodes=args.whole_episode_eval)

    # PPO.learn, with the gate looking in after every iteration
    wall, _ = run_training(ppo, int(algo.get("total_timesteps", 100_000)), after_update=None if gate is None else lambda p, _steps: gate.on_iteration(p, env_cfg),
                           log_every=args.log_every, status=status_line, csv_paths=[root / "progress.csv"])
    if rank != 0:
        return {}
    return _final_artifacts(root, ppo, env_cfg, args=args, resume=resume, n_envs=n_envs * world, world=world, curriculum=curriculum,
                            finisher_policy=finisher_policy, finisher_cfg=finisher_cfg, ws=ws, gate_cfg=gate_cfg, device=local_rank, wall=wall)


def _start_artifacts(root: Path, args, cfg: dict[str, Any]) -> None:
    root.mkdir(parents=True, exist_ok=True)
    (root / "latest_checkpoint").mkdir(exist_ok=True)
    shutil.copyfile(args.config, root / "config_resolved.yaml")
    write_json(root / "training_launch_summary.json", {"run_id": args.run_id, "config": cfg})


def _curriculum_kwargs(cfg: dict[str, Any], env_cfg: kcfg.EnvConfig) -> dict[str, Any] | None:
    """PointCurriculumCallback's settings from the YAML (None: the env has no curriculum stages)"""
    cur = cfg["env"].get("curriculum", {})
    if not (env_cfg.c.curriculum_enabled and env_cfg.n_stages):
        return None
    return {"success_rate_threshold": float(cur.get("success_rate_threshold", 0.80)), "window_episodes": int(cur.get("window_episodes", 20)),
            "min_episodes_per_stage": int(cur.get("min_episodes_per_stage", 30)), "max_stage_index": env_cfg.n_stages - 1}


def _make_curriculum(cfg: dict[str, Any], env_cfg: kcfg.EnvConfig, ws: dict[str, Any], device: int) -> PointCurriculum | None:
    kw = _curriculum_kwargs(cfg, env_cfg)
    if kw is None:
        return None
    return PointCurriculum(**kw, initial_stage_index=int(ws.get("start_stage_index", 0)), device=device)


def _load_finisher(ws: dict[str, Any], device: int):
    if not (ws.get("finisher_checkpoint") and Path(str(ws["finisher_checkpoint"])).exists()):
        return None, None
    from .ppo import InferencePolicy

    finisher_policy = InferencePolicy.load(str(ws["finisher_checkpoint"]), device=device)
    finisher_cfg = kcfg.to_env_config(kcfg.load_yaml_file(ws["finisher_config"]), handoff_base_dirs=(Path(str(ws["finisher_config"])).parent,))
    return finisher_policy, finisher_cfg


def _make_gate(root: Path, env_cfg: kcfg.EnvConfig, finisher_policy, finisher_cfg, ws: dict[str, Any], gate_cfg: dict[str, Any], device: int,
               one_launch: bool | None = None, whole_episodes: bool | None = None) -> WorkspaceEvalGate:
    return WorkspaceEvalGate(artifact_root=root, approach_cfg=env_cfg, finisher_policy=finisher_policy, finisher_cfg=finisher_cfg,
                             eval_interval=int(ws.get("eval_interval", 200_000)), episodes=int(ws.get("gate_eval_episodes", 24)),
                             seed=int(ws.get("eval_seed", 700001)), stage_indices=list(range(env_cfg.n_stages)), gate_config=gate_cfg, device=device,
                             one_launch=one_launch, whole_episodes=whole_episodes)


def _final_artifacts(root: Path, ppo, env_cfg: kcfg.EnvConfig, *, args, resume, n_envs: int, world: int, curriculum, finisher_policy, finisher_cfg,
                     ws: dict[str, Any], gate_cfg: dict[str, Any], device: int, wall: float, extra: dict[str, Any] | None = None,
                     final_eval_payload: dict[str, Any] | None = None) -> dict[str, Any]:
    """what a run leaves at its end: model_latest (twice), the final Approach -> Finisher evaluation when a Finisher is configured, and
    training_summary.json (`ppo` is a PPO or a population replica; ``final_eval_payload``: this replica's share of a population's final
    evaluation, already written under root/final_eval)"""
    latest = root / "latest_checkpoint" / "model_latest"
    checkpoint.save(latest, ppo, env_cfg)
    checkpoint.save(root / "model_latest", ppo, env_cfg)
    final_eval = None
    if finisher_policy is not None:   # train_workspace_expansion.py:243-259
        from . import evaluate as ev

        final_eval = final_eval_payload
        if final_eval is None:
            final_eval = ev.evaluate_workspace_expansion(approach_policy=ppo.predict, finisher_policy=finisher_policy, approach_cfg=env_cfg,
                                                         finisher_cfg=finisher_cfg, episodes=int(ws.get("final_eval_episodes", 80)),
                                                         seed=int(ws.get("eval_seed", 700001)), stage_indices=list(range(env_cfg.n_stages)),
                                                         gate_config=gate_cfg, artifact_root=root / "final_eval", device=device, obs_stride=ppo.obs_w,
                                                         one_launch=False if getattr(args, "multi_launch_eval", False) else None,
                                                         whole_episodes=getattr(args, "whole_episode_eval", None))
        final_eval = {k: v for k, v in final_eval.items() if k != "target_rows"}
        for name in ("stage_metrics.json", "workspace_failure_report.json", "best_model_selection_summary.json"):
            if (root / "final_eval" / name).exists():
                shutil.copyfile(root / "final_eval" / name, root / name)
    summary = {
        "policy_type": "approach", "algorithm": "ppo", "run_id": args.run_id, "checkpoint_format": {"layout": "stable-baselines3 zip", "sb3_loadable": False, "finish_with": "tools/finish_sb3_zip.py (needs stable-baselines3==2.8.0)"}, "model_path": str(latest) + ".zip",
        "resume_from": str(resume) if resume else None, "n_envs": n_envs, "device": f"{world}x MI355X",
        "curriculum_summary": curriculum.summary() if curriculum is not None else None,
        "final_workspace_eval": final_eval, "num_timesteps": ppo.num_timesteps, "wall_seconds": wall,
        "env_steps_per_second": ppo.num_timesteps / wall, "last_update_stats": ppo.last_stats, "update_form": ppo.update_form, **(extra or {}),
    }
    write_json(root / "training_summary.json", summary)
    print(json.dumps({"run_id": args.run_id, "artifact_root": str(root), "model_latest": str(latest) + ".zip",
                      "env_steps_per_second": summary["env_steps_per_second"]}, indent=2))
    return summary


def _main_population(args, cfg, env_cfg, algo, ws, root: Path, batch: int, model_kwargs, resume, world: int, device: int) -> dict[str, Any]:
    """--seeds [--sweep]: the replicas train together as one ApproachPopulationPPO -- one env handle of K x n_envs envs and one tracker launch
    per env step for all of them; replica k writes what a --seed s_k run with its overrides writes, under root/<replica name>/ (seed_<s>
    without --sweep).  --resume-from / workspace_expansion.init_approach_checkpoint: a checkpoint zip every replica starts from, or the root
    of an earlier --seeds run (replica k starts from its own directory's model_latest.zip), as a --seed run resumes (weights, Adam state,
    the saved algorithm constants; the step clock starts at zero).  The gate and the final evaluation run once per gate instant for all
    replicas (evaluate_workspace_expansion_population); --per-replica-eval evaluates them one after another."""
    from .curriculum import PointCurriculumPopulation
    from .population import ApproachPopulationPPO, plan_replicas, population_status, population_summary, resolve_resume_population
    from .vec_env import ArmKinematicPopulationVecEnv

    seeds, overrides, names = plan_replicas(args.seeds, args.sweep)
    refuse_population_under_dp(world)
    # refusals before any device work: the replicas, the width, and the checkpoints a population cannot resume together
    resume_paths = resolve_resume_population(resume, seeds, names) if resume and Path(resume).exists() else None
    hidden = checkpoint.hidden_for_run(args.hidden, resume_paths[0] if resume_paths else None)
    roots = [root / n for n in names]
    pcfg = PPOConfig.from_algo_kwargs(model_kwargs, n_steps=args.n_steps, batch_size=batch, hidden=hidden)
    ApproachPopulationPPO._check_population_args(seeds, pcfg, None, None, overrides)
    env = ArmKinematicPopulationVecEnv(env_cfg, seeds, args.n_envs, device=device, repeated_seeds=True)
    kw = _curriculum_kwargs(cfg, env_cfg)
    curriculum = None
    if kw is not None:
        curriculum = PointCurriculumPopulation(**kw, initial_stage_indices=[int(ws.get("start_stage_index", 0))] * len(seeds), device=device)
    from . import monitor as _monitor

    pop = ApproachPopulationPPO(seeds, pcfg, env, curriculum=curriculum, overrides=overrides, monitor=_monitor.cli_monitor(args))
    if resume_paths is not None:
        pop.load_init_checkpoints(resume_paths, restore_timesteps=False)
        print(f"Resuming workspace expansion of every replica from {resume}")
    for r in roots:
        _start_artifacts(r, args, cfg)
    finisher_policy, finisher_cfg = _load_finisher(ws, device)
    gate_cfg = dict(ws.get("gate", {}) or {})
    gates = {}
    if not args.no_gate_callback and finisher_policy is not None:
        gates = {k: _make_gate(roots[k], env_cfg, finisher_policy, finisher_cfg, ws, gate_cfg, device, whole_episodes=args.whole_episode_eval)
                 for k in range(len(seeds))}

    fused_eval = not args.per_replica_eval

    def on_iteration(p, _steps) -> None:
        if gates and fused_eval:
            population_gate_iteration(gates, p, env_cfg)
            return
        for k in range(len(seeds)):
            if k in gates:
                gates[k].on_iteration(p.replica(k), env_cfg)

    tag = "ppo-population"
    wall, _ = run_training(pop, int(algo.get("total_timesteps", 100_000)), after_update=on_iteration, log_every=args.log_every,
                           status=functools.partial(population_status, tag=tag), csv_paths=[r / "progress.csv" for r in roots], tag=tag)
    rows = []
    finals: list[Any] = [None] * len(seeds)
    if finisher_policy is not None and fused_eval:      # the final evaluation of every replica: one population evaluation
        from . import evaluate as ev

        finals = ev.evaluate_workspace_expansion_population(population=pop, finisher_policy=finisher_policy, approach_cfg=env_cfg, finisher_cfg=finisher_cfg,
                                                            episodes=int(ws.get("final_eval_episodes", 80)), seed=int(ws.get("eval_seed", 700001)),
                                                            stage_indices=list(range(env_cfg.n_stages)), gate_config=gate_cfg,
                                                            artifact_roots=[r / "final_eval" for r in roots], device=device,
                                                            whole_episodes=getattr(args, "whole_episode_eval", None))
    for k, s in enumerate(seeds):
        rep = pop.replica(k)
        summ = _final_artifacts(roots[k], rep, env_cfg, args=args, resume=resume_paths[k] if resume_paths else None, n_envs=args.n_envs, world=1,
                                curriculum=pop.curricula[k], finisher_policy=finisher_policy, finisher_cfg=finisher_cfg, ws=ws, gate_cfg=gate_cfg,
                                device=device, wall=wall, extra=replica_extra(s, names[k], None if overrides is None else overrides[k]), final_eval_payload=finals[k])
        best = gates[k].best_score if k in gates and gates[k].best_score != float("-inf") else None
        rows.append({"seed": s, "artifact_root": str(roots[k]), "final_curriculum_stage": pop.curricula[k].read().stage_index if pop.curricula[k] else None,
                     "last_update_stats": summ["last_update_stats"], "best_score": best, "model_latest": summ["model_path"],
                     "model_best_by_gate": str(roots[k] / "best_checkpoint" / "model_best_by_gate.zip") if best is not None else None})
    summary = population_summary(pop, rows, wall_seconds=wall, selection="workspace eval gate score (best_model_selection.score)")
    write_json(root / "population_summary.json", summary)
    pop.close()
    if curriculum is not None:
        curriculum.close()
    env.close()
    return summary


if __name__ == "__main__":  # pragma: no cover
    main()
