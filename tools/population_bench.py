#!/usr/bin/env python3
"""Population PPO at the reference's training scale (developer tool, not bench.py).

The Approach iteration of workspace_expansion_bigtrain.yaml as the reference trains it -- 16 envs x 1024 steps, minibatch 256, the 2x64 net,
curriculum on -- for a population of K seeds (rl_brain_trainer_amd/population.py), K in {1, 2, 4, 8}.  Per K: rollout ms and update ms per
iteration (device-synchronised, captured graphs), aggregate env-steps/s over all replicas, and the in-situ per-launch duration of the
optimiser-step kernels KP1_MLP_OPT_PROFILE times on this path (grad_finalize, adam) from one eager update.

    python tools/population_bench.py [--ks 1,2,4,8] [--iters 3] [--out profiles/r04_population_refscale.json]

--one-handle: the same Approach iteration as an ApproachPopulationPPO: one env handle of K x 16 envs and one PointCurriculumPopulation, so
every env step is one env launch and one tracker launch for all replicas (K in {1, 2, 4, 8, 16} by default).  Without it every replica has
its own handle and tracker (PopulationPPO), which is the comparison.

    python tools/population_bench.py --one-handle [--ks 1,2,4,8,16] [--out profiles/r06_approach_population_refscale.json]

--route: the route reference-scale iteration instead -- route_curriculum_prefix120_routeobs_sequence2 on tests/golden/synthetic_route.json,
16 envs x 1024 steps, minibatch 512, 2x64, graphs on -- as a RoutePopulationPPO: one route env handle of K x 16 envs and one tracker launch
per env step for all replicas (K in {1, 2, 4, 8, 16} by default).

    python tools/population_bench.py --route [--ks 1,2,4,8,16] [--out profiles/r05_route_population_refscale.json]

--dock: the Finisher's reference shape -- the dock_workspace_handoff_noop_ft_12env iteration with the handoff-state buffer of tests/golden,
12 envs x 256 steps per replica, minibatch 256, 2x64, graphs on -- measured both ways for every K (K in {1, 2, 4, 8, 16} by default): as a
DockPopulationPPO (one env handle of K x 12 envs and one DockReverseCurriculumPopulation launch per env step) and as the K-handle
PopulationPPO (one handle and one DockReverseCurriculum per replica).  No shipped YAML has a reverse curriculum, so the tracker runs a small
synthetic stage table (DOCK_STAGES); --no-curriculum measures the plain dock step without a tracker.

    python tools/population_bench.py --dock [--no-curriculum] [--ks 1,2,4,8,16] [--out profiles/r07_dock_population_refscale.json]

--eval: the wall time of one gate evaluation of a --seeds run -- n_stages x 24 episodes of workspace_expansion_bigtrain, Approach then
Finisher (a freshly initialised 2x64 Finisher on dock_workspace_handoff_noop_ft_12env: the reference's checkpoint is not shipped) -- for an
ApproachPopulationPPO of K replicas after one training iteration, both ways, alternately in one process, --repeats times each: K sequential
evaluate_workspace_expansion calls through replica(k).predict (per_replica) and one evaluate_workspace_expansion_population (population).
Also the iteration time at the reference scale, and from both the share of a run's wall time that gate evaluation takes at the shipped
eval_interval.

    python tools/population_bench.py --eval [--ks 1,8,16] [--repeats 5] [--out profiles/r09_population_eval.json]

--route-eval: the wall time of the final sequential evaluations of a `train_route --seeds` run -- the default gate's prefixes up to
--end-index plus the full route taken as --end-index (40: prefixes 20 and 40, then 40 again) -- for a RoutePopulationPPO of K replicas after
one training iteration of the --route shape, both ways, alternately in one process, --repeats times each: K x (prefixes + full)
evaluate_sequential_route calls through replica(k).predict (per_replica) and one evaluate_sequential_route_batch with one chain per replica,
every evaluation a slice of it (batch).  Also the batch form's time per lock step.

    python tools/population_bench.py --route-eval [--ks 1,8,16] [--end-index 40] [--repeats 5] [--out profiles/r10_route_population_eval.json]

--route-anchor: the teacher-anchor side loss of a `train_route --seeds` run at the --route shape (minibatch 512, anchor batch 256, one
gradient step after every rollout) on a servo dataset recorded from the device env: the wall time of one training iteration of a
RoutePopulationPPO of K replicas without and with a PopulationTeacherAnchor, the time of one device anchor step (all K replicas), and the
time of RouteTeacherAnchor.gradient_step (torch autograd + repack) on one single PPO in the same process -- K times that is what training
the seeds one by one pays per rollout.  The variants alternate, --repeats times each; median and max - min are reported.

    python tools/population_bench.py --route-anchor [--ks 1,8,16] [--repeats 5] [--out profiles/r11_route_anchor.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from rl_brain_trainer_amd import config as kcfg  # noqa: E402
from rl_brain_trainer_amd.curriculum import PointCurriculum  # noqa: E402
from rl_brain_trainer_amd.population import PopulationPPO  # noqa: E402
from rl_brain_trainer_amd.ppo import PPOConfig  # noqa: E402
from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv  # noqa: E402


def _approach_setup(n_steps: int, batch: int, hidden: int):
    cfg = kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml")
    env_cfg = kcfg.to_env_config(cfg)
    cur = cfg["env"].get("curriculum", {})
    algo = {k: v for k, v in kcfg.to_algorithm_kwargs(cfg, "ppo").items() if k not in ("total_timesteps", "n_steps", "batch_size", "seed")}
    pcfg = PPOConfig.from_algo_kwargs(algo, n_steps=n_steps, batch_size=batch, hidden=hidden)
    tracker = None
    if env_cfg.c.curriculum_enabled and env_cfg.n_stages:
        tracker = {"success_rate_threshold": float(cur.get("success_rate_threshold", 0.80)), "window_episodes": int(cur.get("window_episodes", 20)),
                   "min_episodes_per_stage": int(cur.get("min_episodes_per_stage", 30)), "max_stage_index": env_cfg.n_stages - 1}
    return env_cfg, pcfg, tracker


def build_approach(K: int, n_envs: int, n_steps: int, batch: int, hidden: int, use_graphs: bool) -> PopulationPPO:
    env_cfg, pcfg, tracker = _approach_setup(n_steps, batch, hidden)
    return PopulationPPO(list(range(7, 7 + K)), pcfg, lambda s: ArmKinematicVecEnv(env_cfg, n_envs, seed=s),
                         curriculum_factory=lambda s: PointCurriculum(**tracker) if tracker else None, use_graphs=use_graphs)


SWEEP: list[tuple[str, list[float]]] = []     # --sweep: replica k takes value k % len(values) of every swept key
MONITOR = [False]     # --monitor: the --one-handle and --single-seed iterations with the training monitor on (monitor.py)


def _sweep_overrides(K: int) -> list[dict[str, float]] | None:
    return [{key: vals[k % len(vals)] for key, vals in SWEEP} for k in range(K)] if SWEEP else None


def build_approach_one_handle(K: int, n_envs: int, n_steps: int, batch: int, hidden: int, use_graphs: bool) -> PopulationPPO:
    from rl_brain_trainer_amd.curriculum import PointCurriculumPopulation
    from rl_brain_trainer_amd.population import ApproachPopulationPPO
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    env_cfg, pcfg, tracker = _approach_setup(n_steps, batch, hidden)
    seeds = list(range(7, 7 + K))
    env = ArmKinematicPopulationVecEnv(env_cfg, seeds, n_envs)
    cur = PointCurriculumPopulation(**tracker, initial_stage_indices=[0] * K) if tracker else None
    pop = ApproachPopulationPPO(seeds, pcfg, env, curriculum=cur, use_graphs=use_graphs, overrides=_sweep_overrides(K), monitor=MONITOR[0])
    pop._bench_owned = [c for c in (cur, env) if c is not None]     # closed after the population (the caller owns them)
    return pop


def build_single_seed(K: int, n_envs: int, n_steps: int, batch: int, hidden: int, use_graphs: bool):
    """the single-seed trainer on the Approach iteration: PPO(ArmKinematicVecEnv, PointCurriculum), seed 7 (K is 1)"""
    from rl_brain_trainer_amd.ppo import PPO

    assert K == 1, "--single-seed is one PPO run"
    env_cfg, pcfg, tracker = _approach_setup(n_steps, batch, hidden)
    env = ArmKinematicVecEnv(env_cfg, n_envs, seed=7)
    cur = PointCurriculum(**tracker) if tracker else None
    ppo = PPO(env, pcfg, curriculum=cur, use_graphs=use_graphs, monitor=MONITOR[0])
    ppo._bench_owned = [c for c in (cur, env) if c is not None]
    return ppo


ROUTE_CONFIG = ROOT / "tests" / "golden" / "configs" / "route_curriculum_prefix120_routeobs_sequence2.json"
ROUTE_PATH = ROOT / "tests" / "golden" / "synthetic_route.json"


def build_route(K: int, n_envs: int, n_steps: int, batch: int, hidden: int, use_graphs: bool, anchor=None) -> PopulationPPO:
    from rl_brain_trainer_amd import route_config as rcfg
    from rl_brain_trainer_amd.population import RoutePopulationPPO
    from rl_brain_trainer_amd.route_curriculum import RoutePrefixCurriculumPopulation
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv

    cfg = json.loads(ROUTE_CONFIG.read_text())
    route_q = rcfg.load_route_q(ROUTE_PATH)
    prefixes = rcfg.prefix_stages(cfg, int(route_q.shape[0]))
    algo = {k: v for k, v in kcfg.to_algorithm_kwargs(cfg, "ppo").items() if k not in ("total_timesteps", "n_steps", "batch_size", "seed")}
    pcfg = PPOConfig.from_algo_kwargs(algo, n_steps=n_steps, batch_size=batch, hidden=hidden)
    seeds = list(range(7, 7 + K))
    env = RoutePopulationVecEnv(kcfg.to_env_config(cfg), rcfg.route_config_from_dict(cfg, max_route_index=prefixes[0]), route_q, seeds, n_envs)
    cur = RoutePrefixCurriculumPopulation.from_config(cfg, int(route_q.shape[0]))
    pop = RoutePopulationPPO(seeds, pcfg, env, curriculum=cur, use_graphs=use_graphs, teacher_anchor=anchor)
    pop._bench_owned = [cur, env]     # closed after the population (the caller owns a route population's env and tracker)
    return pop


DOCK_CONFIG = ROOT / "tests" / "golden" / "configs" / "dock_workspace_handoff_noop_ft_12env_raw.json"
# a small synthetic reverse curriculum: promotions on episode counts (threshold 0), every overridable value, a per-stage handoff filter
DOCK_STAGES = [
    {"name": "close", "min_episodes": 48, "window_episodes": 12, "success_rate_threshold": 0.0, "dock_residual_action_limit": 0.2,
     "close_bucket_probability": 1.0, "close_bucket_max_pos_error_m": 0.003, "handoff_state_probability": 0.3},
    {"name": "mid", "min_episodes": 96, "success_rate_threshold": 0.0, "action_delta_scale": 0.012, "close_bucket_probability": 0.5,
     "handoff_state_probability": 0.6, "handoff_state_max_action_l2": 0.3},
    {"name": "wide", "dock_delta_q_change_limit_scale": 0.5, "dock_residual_action_limit": 0.35, "close_bucket_probability": 0.15,
     "handoff_state_probability": 0.95},
]


def _dock_setup(n_steps: int, batch: int, hidden: int):
    cfg = json.loads(DOCK_CONFIG.read_text())
    env_cfg = kcfg.to_env_config(cfg, handoff_base_dirs=(DOCK_CONFIG.parents[1],))
    algo = {k: v for k, v in kcfg.to_algorithm_kwargs(cfg, "ppo").items() if k not in ("total_timesteps", "n_steps", "batch_size", "seed")}
    return env_cfg, PPOConfig.from_algo_kwargs(algo, n_steps=n_steps, batch_size=batch, hidden=hidden)


def build_dock_one_handle(K: int, n_envs: int, n_steps: int, batch: int, hidden: int, use_graphs: bool, curriculum: bool) -> PopulationPPO:
    from rl_brain_trainer_amd.finisher_tools import DockReverseCurriculumPopulation
    from rl_brain_trainer_amd.population import DockPopulationPPO
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    env_cfg, pcfg = _dock_setup(n_steps, batch, hidden)
    seeds = list(range(7, 7 + K))
    env = ArmKinematicPopulationVecEnv(env_cfg, seeds, n_envs, mode="dock")
    cur = None
    if curriculum:
        cur = DockReverseCurriculumPopulation(stages=DOCK_STAGES, window_episodes=12, n_replicas=K, handoff_base_dirs=(DOCK_CONFIG.parents[1],))
    pop = DockPopulationPPO(seeds, pcfg, env, curriculum=cur, use_graphs=use_graphs)
    pop._bench_owned = [c for c in (cur, env) if c is not None]
    return pop


def build_dock_k_handles(K: int, n_envs: int, n_steps: int, batch: int, hidden: int, use_graphs: bool, curriculum: bool) -> PopulationPPO:
    from rl_brain_trainer_amd.finisher_tools import DockReverseCurriculum

    def make_cur(_s):
        return DockReverseCurriculum(stages=DOCK_STAGES, window_episodes=12, handoff_base_dirs=(DOCK_CONFIG.parents[1],)) if curriculum else None

    # every replica its own config object: a single tracker writes its stage into its handle's config
    _, pcfg = _dock_setup(n_steps, batch, hidden)
    return PopulationPPO(list(range(7, 7 + K)), pcfg, lambda s: ArmKinematicVecEnv(_dock_setup(n_steps, batch, hidden)[0], n_envs, seed=s),
                         curriculum_factory=make_cur, use_graphs=use_graphs)


def _close(pop) -> None:
    if hasattr(pop, "close"):
        pop.close()
    else:
        pop._mlp.close()     # a single PPO has no close() of its own
    for obj in getattr(pop, "_bench_owned", []):
        obj.close()


def measure(K: int, args, build=None) -> dict:
    build = build or (build_route if args.route else build_single_seed if args.single_seed else
                      (build_approach_one_handle if args.one_handle else build_approach))
    pop = build(K, args.n_envs, args.n_steps, args.batch, args.hidden, True)
    pop.collect_rollouts()
    pop.train()      # warm-up: captures both graphs
    torch.cuda.synchronize()
    ro, up = [], []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        pop.collect_rollouts()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        pop.train()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ro.append(t1 - t0)
        up.append(t2 - t1)
    rollout_ms, update_ms = 1e3 * sum(ro) / len(ro), 1e3 * sum(up) / len(up)
    steps = K * args.n_envs * args.n_steps
    ro_sorted = sorted(1e3 * v for v in ro)
    rollout_stats = {"rollout_ms_median": ro_sorted[len(ro_sorted) // 2], "rollout_ms_spread": ro_sorted[-1] - ro_sorted[0],
                     "us_per_env_step": 1e3 * ro_sorted[len(ro_sorted) // 2] / args.n_steps}   # one env step = one step of all K x n_envs envs
    _close(pop)
    # per-kernel durations from one eager update with event pairs on the launches
    eager = build(K, args.n_envs, args.n_steps, args.batch, args.hidden, False)
    eager.collect_rollouts()
    torch.cuda.synchronize()
    eager._mlp.set_profile(True)
    eager.train()
    prof = {k: v for k, v in eager._mlp.profile_read().items() if v["launches"] > 0}
    eager._mlp.set_profile(False)
    _close(eager)
    return {"K": K, "rollout_ms": rollout_ms, "update_ms": update_ms, "iteration_ms": rollout_ms + update_ms,
            "aggregate_env_steps_per_s": steps / ((rollout_ms + update_ms) * 1e-3), "env_steps_per_iteration": steps, "kernel_us_in_situ": prof,
            **rollout_stats}


def main_eval(args) -> None:
    import statistics

    from rl_brain_trainer_amd import evaluate as ev
    from rl_brain_trainer_amd.ppo import ActorCritic, InferencePolicy

    args.ks = args.ks or "1,8,16"
    args.batch = args.batch or 256
    cfg = kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml")
    ws = cfg.get("workspace_expansion", {})
    env_cfg = kcfg.to_env_config(cfg)
    dock = kcfg.load_yaml_file(kcfg.builtin_config_dir() / "dock_workspace_handoff_noop_ft_12env.yaml")
    dock["env"]["dock_reset"]["handoff_state_probability"] = 0.0      # the reference's handoff buffer file is not shipped
    fcfg = kcfg.to_env_config(dock)
    dev = torch.device("cuda", 0)
    fin = InferencePolicy(ActorCritic(64, dev, seed=1).state_dict(), device=dev)
    episodes, interval = int(ws.get("gate_eval_episodes", 24)), int(ws.get("eval_interval", 200_000))
    kw = dict(finisher_policy=fin, approach_cfg=env_cfg, finisher_cfg=fcfg, episodes=episodes, seed=int(ws.get("eval_seed", 700001)),
              stage_indices=list(range(env_cfg.n_stages)), gate_config=dict(ws.get("gate", {}) or {}), handoff_confirm_steps=args.handoff_confirm_steps)

    def timed(fn) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    rows = []
    for K in (int(k) for k in args.ks.split(",")):
        pop = build_approach_one_handle(K, args.n_envs, args.n_steps, args.batch, args.hidden, True)
        pop.collect_rollouts()
        pop.train()      # warm-up: captures both graphs, and the replicas' weights differ
        iters = [timed(lambda: (pop.collect_rollouts(), pop.train())) for _ in range(args.iters)]

        def per_replica():
            for k in range(K):
                ev.evaluate_workspace_expansion(approach_policy=pop.replica(k).predict, obs_stride=pop.obs_w, **kw)

        def population():
            return ev.evaluate_workspace_expansion_population(population=pop, **kw)

        per_replica()                    # warm-up of both forms
        # rows that hand over to the Finisher (the Finisher phase steps all rows while any of them is alive)
        handoffs = sum(bool(r["finisher_ready_dwell"]) for p in population() for r in p["target_rows"])
        t = {"per_replica": [], "population": []}
        for _ in range(args.repeats):
            t["per_replica"].append(timed(per_replica))
            t["population"].append(timed(population))
        _close(pop)
        iteration_ms = statistics.median(iters)
        # evaluations land on iteration boundaries: one per ceil(eval_interval / steps per iteration) iterations
        iters_per_eval = -(-interval // (args.n_envs * args.n_steps))
        row = {"K": K, "episodes": env_cfg.n_stages * episodes, "handoff_confirm_steps": args.handoff_confirm_steps,
               "handoff_rows_of_all_replicas": handoffs, "iteration_ms": iteration_ms, "iterations_per_evaluation": iters_per_eval}
        for form, ms in t.items():
            med = statistics.median(ms)
            row[form] = {"ms": ms, "median_ms": med, "spread_ms": max(ms) - min(ms),
                         "share_of_run_wall_time": med / (med + iters_per_eval * iteration_ms)}
        row["speedup_median"] = row["per_replica"]["median_ms"] / row["population"]["median_ms"]
        row["faster_by_more_than_per_replica_spread"] = row["per_replica"]["median_ms"] - row["population"]["median_ms"] > row["per_replica"]["spread_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"workload": f"one gate evaluation of workspace_expansion_bigtrain ({env_cfg.n_stages} stages x {episodes} episodes, Approach + a fresh 2x64 "
                          f"Finisher on dock_workspace_handoff_noop_ft_12env) of an ApproachPopulationPPO, {args.n_envs} envs x {args.n_steps} steps per "
                          f"replica, minibatch {args.batch}, 2x{args.hidden}, after one iteration; per_replica = K evaluate_workspace_expansion calls "
                          f"through replica(k).predict, population = one evaluate_workspace_expansion_population; alternated, {args.repeats} repeats; "
                          f"handoff_confirm_steps {args.handoff_confirm_steps}; "
                          f"share_of_run_wall_time = evaluation / (evaluation + iterations_per_evaluation x iteration) at eval_interval {interval}",
              "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=2) + "\n")
    print(json.dumps({"gate_evaluation_median_ms": {r["K"]: {f: round(r[f]["median_ms"], 1) for f in ("per_replica", "population")} for r in rows}}))


def main_route_eval(args) -> None:
    import statistics

    from rl_brain_trainer_amd import route_config as rcfg
    from rl_brain_trainer_amd.route_curriculum import evaluate_sequential_route, evaluate_sequential_route_batch, sliced_evaluate

    args.ks = args.ks or "1,8,16"
    args.batch = args.batch or 512
    cfg = json.loads(ROUTE_CONFIG.read_text())
    route_q = rcfg.load_route_q(ROUTE_PATH)
    E = int(args.end_index)
    ends = [p for p in (20, 40, 80, 120, 180) if p <= E] + [E]      # the default gate's prefixes inside the bound, then the "full route"

    def timed(fn) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    rows = []
    for K in (int(k) for k in args.ks.split(",")):
        pop = build_route(K, args.n_envs, args.n_steps, args.batch, args.hidden, True)
        pop.collect_rollouts()
        pop.train()      # one training iteration: the replicas' weights differ
        torch.cuda.synchronize()
        progress = pop.pop_env.route_progress_m
        seen = {}

        def per_replica():
            out = []
            for k in range(K):
                policy = pop.replica(k).predict
                out.append([evaluate_sequential_route(policy=lambda o: policy(o.float().contiguous()), cfg=cfg, route_q=route_q, start_index=1, end_index=e)
                            for e in ends])
            seen["per_replica"] = out

        def batch():
            chains = evaluate_sequential_route_batch(mlp=pop._mlp, cfg=cfg, route_q=route_q, start_index=1, end_indices=[E] * K)
            seen["lock_steps"] = chains[0]["lock_steps"]
            seen["batch"] = [[sliced_evaluate(c["rows"], c["final_qs"], progress)(artifact_root=None, start_index=1, end_index=e) for e in ends] for c in chains]

        per_replica()      # warm-up of both forms; the two forms must agree before either is timed
        batch()
        for k in range(K):
            for a, b in zip(seen["per_replica"][k], seen["batch"][k]):
                assert {key: a[key] for key in b} == b, (K, k)
        t = {"per_replica": [], "batch": []}
        for _ in range(args.repeats):
            t["per_replica"].append(timed(per_replica))
            t["batch"].append(timed(batch))
        _close(pop)
        row = {"K": K, "end_index": E, "evaluations_per_replica": ends, "waypoint_episodes_per_replica": {"per_replica": sum(ends), "batch": E},
               "lock_steps": seen["lock_steps"]}
        for form, ms in t.items():
            med = statistics.median(ms)
            row[form] = {"ms": ms, "median_ms": med, "spread_ms": max(ms) - min(ms)}
        row["batch"]["us_per_lock_step"] = 1e3 * row["batch"]["median_ms"] / max(seen["lock_steps"], 1)
        row["speedup_median"] = row["per_replica"]["median_ms"] / row["batch"]["median_ms"]
        row["faster_by_more_than_per_replica_spread"] = row["per_replica"]["median_ms"] - row["batch"]["median_ms"] > row["per_replica"]["spread_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"workload": f"final sequential evaluations of a train_route --seeds run on synthetic_route.json (route_curriculum_prefix120_routeobs_sequence2), "
                          f"end indices {ends} per replica (the default gate's prefixes up to {E}, then the full route taken as {E}), for a "
                          f"RoutePopulationPPO of K replicas, {args.n_envs} envs x {args.n_steps} steps per replica, minibatch {args.batch}, 2x{args.hidden}, "
                          f"after one iteration; per_replica = K x {len(ends)} evaluate_sequential_route calls through replica(k).predict, batch = one "
                          f"evaluate_sequential_route_batch (one chain per replica to {E}) + {len(ends)} slices per replica; alternated, {args.repeats} "
                          "repeats; no artifact files in either form",
              "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=2) + "\n")
    print(json.dumps({"route_evaluation_median_ms": {r["K"]: {f: round(r[f]["median_ms"], 1) for f in ("per_replica", "batch")} for r in rows}}))


def main_route_chain_forms(args) -> None:
    """--route-eval --chain-form: the chained evaluation's forms against each other (the launch sequence is the reference IN THE SAME RUN), the
    whole-chain form once per --steps-per-launch value; results asserted equal before anything is timed, then alternated in one process"""
    import statistics

    from rl_brain_trainer_amd import route_config as rcfg
    from rl_brain_trainer_amd.route_curriculum import evaluate_sequential_route_batch

    args.ks = args.ks or "1,8,16"
    args.batch = args.batch or 512
    cfg = json.loads(ROUTE_CONFIG.read_text())
    route_q = rcfg.load_route_q(ROUTE_PATH)
    E = int(args.end_index)
    forms = [f.strip().replace("-", "_") for f in args.chain_form.split(",")]
    spans = [int(v) for v in args.steps_per_launch.split(",")]
    legs = []
    for f in forms:
        legs += [(f"{f}@{sp}", f, sp) for sp in spans] if f == "whole_chain" else [(f, f, 32)]
    if "launch_sequence" not in forms:
        legs.insert(0, ("launch_sequence", "launch_sequence", 32))

    rows = []
    for K in (int(k) for k in args.ks.split(",")):
        pop = build_route(K, args.n_envs, args.n_steps, args.batch, args.hidden, True)
        pop.collect_rollouts()
        pop.train()      # one training iteration: the replicas' weights differ
        torch.cuda.synchronize()
        seen = {}

        def run(name, form, span):
            chains = evaluate_sequential_route_batch(mlp=pop._mlp, cfg=cfg, route_q=route_q, start_index=1, end_indices=[E] * K, form=form,
                                                     steps_per_launch=span)
            seen[name] = chains

        def timed(leg) -> float:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(*leg)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0)

        for leg in legs:      # warm-up of every leg; all must agree with the launch sequence before any is timed
            run(*leg)
        ref = seen["launch_sequence"]
        for name, _, span in legs:
            for a, b in zip(seen[name], ref):
                assert {k: v for k, v in a.items() if k != "lock_steps"} == {k: v for k, v in b.items() if k != "lock_steps"}, (K, name)
                assert span > 32 or a["lock_steps"] == b["lock_steps"], (K, name, a["lock_steps"], b["lock_steps"])
        t = {name: [] for name, _, _ in legs}
        for _ in range(args.repeats):
            for leg in legs:
                t[leg[0]].append(timed(leg))
        _close(pop)
        row = {"K": K, "end_index": E}
        for name, _, _ in legs:
            ms = t[name]
            steps = seen[name][0]["lock_steps"]
            med = statistics.median(ms)
            row[name] = {"ms": ms, "median_ms": med, "spread_ms": max(ms) - min(ms), "lock_steps": steps, "us_per_lock_step": 1e3 * med / max(steps, 1)}
        base = row["launch_sequence"]
        for name, _, _ in legs[1:] if legs[0][0] == "launch_sequence" else legs:
            if name != "launch_sequence":
                row[name]["beats_launch_sequence_by_more_than_its_spread"] = base["median_ms"] - row[name]["median_ms"] > base["spread_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"workload": f"chained final evaluation of a train_route --seeds run on synthetic_route.json (route_curriculum_prefix120_routeobs_sequence2): "
                          f"one chain per replica to waypoint {E}, RoutePopulationPPO of K replicas, {args.n_envs} envs x {args.n_steps} steps per replica, "
                          f"minibatch {args.batch}, 2x{args.hidden}, after one iteration; evaluate_sequential_route_batch(form=...), whole_chain@S = "
                          f"steps_per_launch S; results equal before timing; legs alternated in one process, one warm-up, {args.repeats} repeats; host "
                          "clock around a device synchronise; no artifact files",
              "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=2) + "\n")
    print(json.dumps({"route_chain_median_ms": {r["K"]: {n: round(r[n]["median_ms"], 1) for n, _, _ in legs} for r in rows}}))


def _record_servo_dataset(path: Path, max_route_index: int) -> None:
    """a teacher-anchor dataset as collect_route_teacher writes it: 64 device envs under a servo toward the route goal, 32 steps"""
    import numpy as np

    from rl_brain_trainer_amd import route_config as rcfg
    from rl_brain_trainer_amd.route_env import RouteVecEnv

    cfg = json.loads(ROUTE_CONFIG.read_text())
    env = RouteVecEnv(kcfg.to_env_config(cfg), rcfg.route_config_from_dict(cfg, max_route_index=max_route_index), rcfg.load_route_q(ROUTE_PATH), 64, seed=3)
    rows, acts, ridx = [], [], []
    obs = env.reset()
    for _ in range(32):
        a = (0.8 * RouteVecEnv.obs_dict(obs)["route_q_error"]).clamp(-1, 1)
        rows.append(obs[:, :env.obs_dim].cpu().numpy().copy())
        acts.append(a.cpu().numpy().copy())
        ridx.append(env.info()["route_index"].cpu().numpy().copy())
        obs, _, _ = env.step(a)
    env.close()
    rows, acts, ridx = np.concatenate(rows), np.concatenate(acts), np.concatenate(ridx)
    np.savez(path, actions=acts.astype(np.float32), route_index=ridx.astype(np.int32),
             **{f"obs__{k}": rows[:, o:o + w] for k, (o, w) in rcfg.ROUTE_OBS_LAYOUT.items()})


def main_route_anchor(args) -> None:
    import statistics
    import tempfile

    from rl_brain_trainer_amd import route_config as rcfg
    from rl_brain_trainer_amd.ppo import PPO
    from rl_brain_trainer_amd.route_env import RouteVecEnv
    from rl_brain_trainer_amd.teacher_anchor import PopulationTeacherAnchor, RouteTeacherAnchor, TeacherAnchorConfig

    args.ks = args.ks or "1,8,16"
    args.batch = args.batch or 512
    STEPS = 20     # anchor steps per timed repeat

    def timed(fn) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def stat(ms: list[float], scale: float = 1.0) -> dict:
        v = [x * scale for x in ms]
        return {"values": v, "median": statistics.median(v), "spread": max(v) - min(v)}

    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        npz = Path(tmp) / "teacher_route_anchor_dataset.npz"
        _record_servo_dataset(npz, 40)
        acfg = TeacherAnchorConfig(enabled=True, dataset_path=str(npz), loss_weight=0.02, batch_size=256, max_route_index=40)
        # the parent's step: one single PPO of the same shape, RouteTeacherAnchor (torch autograd on the flat vector, then a full repack)
        cfg = json.loads(ROUTE_CONFIG.read_text())
        route_q = rcfg.load_route_q(ROUTE_PATH)
        algo = {k: v for k, v in kcfg.to_algorithm_kwargs(cfg, "ppo").items() if k not in ("total_timesteps", "n_steps", "batch_size", "seed")}
        senv = RouteVecEnv(kcfg.to_env_config(cfg), rcfg.route_config_from_dict(cfg, max_route_index=rcfg.prefix_stages(cfg, int(route_q.shape[0]))[0]),
                           route_q, args.n_envs, seed=7)
        single = PPO(senv, PPOConfig.from_algo_kwargs(algo, n_steps=args.n_steps, batch_size=args.batch, hidden=args.hidden))
        single.collect_rollouts()
        single.train()
        sanchor = RouteTeacherAnchor(acfg)
        sanchor.on_training_start(single)

        def torch_steps():
            for _ in range(STEPS):
                pick = torch.as_tensor(sanchor.sample_indices(), device=single.device)
                sanchor.gradient_step(single, sanchor._obs.index_select(0, pick), sanchor._actions.index_select(0, pick))

        torch_steps()      # warm-up
        for K in (int(k) for k in args.ks.split(",")):
            anchor = PopulationTeacherAnchor(acfg)
            on = build_route(K, args.n_envs, args.n_steps, args.batch, args.hidden, True, anchor=anchor)
            off = build_route(K, args.n_envs, args.n_steps, args.batch, args.hidden, True)

            def iteration(pop, a=None):
                pop.collect_rollouts()
                if a is not None:
                    a.on_rollout_end(pop)
                pop.train()

            def device_steps():
                for _ in range(STEPS):
                    anchor.gradient_step(on, anchor.sample_indices())

            for _ in range(2):      # warm-up: both graphs of both populations captured, the anchor kernels loaded
                iteration(off)
                iteration(on, anchor)
            device_steps()
            t = {"iteration_anchor_off_ms": [], "iteration_anchor_on_ms": [], "device_anchor_step": [], "torch_anchor_step": []}
            for _ in range(args.repeats):
                t["iteration_anchor_off_ms"].append(timed(lambda: iteration(off)))
                t["iteration_anchor_on_ms"].append(timed(lambda: iteration(on, anchor)))
                t["device_anchor_step"].append(timed(device_steps))
                t["torch_anchor_step"].append(timed(torch_steps))
            row = {"K": K, "anchor_rows": anchor.batch_rows, "anchor_steps_per_timed_repeat": STEPS,
                   "iteration_anchor_off_ms": stat(t["iteration_anchor_off_ms"]), "iteration_anchor_on_ms": stat(t["iteration_anchor_on_ms"]),
                   "device_anchor_step_us": stat(t["device_anchor_step"], 1e3 / STEPS),             # all K replicas
                   "torch_anchor_step_single_ppo_us": stat(t["torch_anchor_step"], 1e3 / STEPS)}    # one replica
            row["one_by_one_anchor_us_per_rollout"] = K * row["torch_anchor_step_single_ppo_us"]["median"]
            row["anchor_cost_in_iteration_ms"] = row["iteration_anchor_on_ms"]["median"] - row["iteration_anchor_off_ms"]["median"]
            gain = row["one_by_one_anchor_us_per_rollout"] - row["device_anchor_step_us"]["median"]
            row["device_step_faster_by_more_than_spread"] = gain > K * row["torch_anchor_step_single_ppo_us"]["spread"] + row["device_anchor_step_us"]["spread"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            _close(on)
            _close(off)
        senv.close()
    result = {"workload": f"teacher-anchor side loss at the --route shape: route_curriculum_prefix120_routeobs_sequence2 on synthetic_route.json, "
                          f"{args.n_envs} envs x {args.n_steps} steps per replica, minibatch {args.batch}, 2x{args.hidden}, graphs on, anchor batch 256 on a "
                          f"servo dataset of the device env, one gradient step per rollout; iteration = collect_rollouts [+ anchor] + train, "
                          f"device-synchronised; anchor step times are means over {STEPS} consecutive steps; variants alternated, {args.repeats} repeats, "
                          "median and spread = max - min; torch_anchor_step_single_ppo = RouteTeacherAnchor.gradient_step on ONE PPO",
              "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=2) + "\n")
    print(json.dumps({"anchor_step_us": {r["K"]: {"device_all_replicas": round(r["device_anchor_step_us"]["median"], 1),
                                                  "torch_one_replica": round(r["torch_anchor_step_single_ppo_us"]["median"], 1)} for r in rows}}))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--route-anchor", action="store_true", help="the teacher-anchor side loss of a route --seeds run: iteration time without and "
                    "with the device anchor step, and the device step against the torch step of one single PPO")
    ap.add_argument("--route-eval", action="store_true", help="the final sequential evaluations of a route --seeds run: K x (prefixes + full) "
                    "per-replica evaluations against one chained batch evaluation")
    ap.add_argument("--chain-form", default=None, help="with --route-eval: comma list of launch-sequence, one-launch-step, whole-chain -- time the "
                    "chained evaluation's forms against the launch sequence in one process (the per-replica form is not run)")
    ap.add_argument("--steps-per-launch", default="32", help="with --chain-form whole-chain: comma list of lock steps per launch (1 .. 1024)")
    ap.add_argument("--end-index", type=int, default=40, help="with --route-eval: the largest route index evaluated (the 'full route' of the bench)")
    ap.add_argument("--eval", action="store_true", help="one gate evaluation of a --seeds run: K per-replica evaluations against one population evaluation")
    ap.add_argument("--repeats", type=int, default=5, help="with --eval: timed repeats of each form")
    ap.add_argument("--handoff-confirm-steps", type=int, default=2, help="with --eval: the evaluator's handoff_confirm_steps (2, the gate's; 0 hands "
                    "every episode over at step 1, so the Finisher phase runs over all rows whatever the policy has learnt)")
    ap.add_argument("--route", action="store_true", help="the route reference-scale iteration (RoutePopulationPPO)")
    ap.add_argument("--one-launch-rollout", action="store_true", help="with --route: every rollout step as one launch (sets "
                    "KP1_FUSED_ROUTE_ROLLOUT=1: kp1_mlp_forward_route_step, DESIGN section 22); default: the launch sequence")
    ap.add_argument("--one-handle", action="store_true", help="the Approach iteration on one env handle (ApproachPopulationPPO)")
    ap.add_argument("--single-seed", action="store_true", help="the Approach iteration of the single-seed trainer (PPO, one env handle, K = 1)")
    ap.add_argument("--rollout-form", choices=("per-step", "whole"), default=None, help="with --one-handle or --single-seed: the rollout as one "
                    "launch sequence per env step (sets KP1_ROLLOUT_RUN=0) or as one launch per span of env steps (KP1_ROLLOUT_RUN=1: "
                    "kp1_rollout_run, DESIGN section 27); default: the trainer's own choice")
    ap.add_argument("--train-tile", action="store_true", help="hidden 64 / 128: the optimiser step's forward, loss and backward as one tile launch "
                    "(train_tile128_kernel; sets KP1_TRAIN_TILE=1, which every trainer class reads when it creates its MLP handle)")
    ap.add_argument("--dock", action="store_true", help="the Finisher reference shape, one handle (DockPopulationPPO) and K handles")
    ap.add_argument("--no-curriculum", action="store_true", help="with --dock: no reverse-curriculum tracker")
    ap.add_argument("--ks", default="")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--n-envs", type=int, default=0, help="envs per replica (0 = 16, or 12 with --dock)")
    ap.add_argument("--n-steps", type=int, default=0, help="steps per rollout (0 = 1024, or 256 with --dock)")
    ap.add_argument("--batch", type=int, default=0, help="minibatch (0 = 256, or 512 with --route)")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--sweep", action="append", metavar="KEY=v1,v2", help="with --one-handle: per-replica hyper-parameters (replica k takes value "
                    "k %% n of each key; the per-replica table and GAE scan of a population with overrides)")
    ap.add_argument("--monitor", action="store_true", help="with --one-handle or --single-seed: the training monitor on (two launches in front of "
                    "the rollout tail, one behind it, and the log_std copy after the update)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.monitor:
        if not (args.one_handle or args.single_seed):
            ap.error("--monitor is measured on the --one-handle and --single-seed Approach iterations")
        MONITOR[0] = True
    if args.sweep:
        from rl_brain_trainer_amd.population import parse_sweep

        if not args.one_handle:
            ap.error("--sweep is measured on the --one-handle Approach iteration")
        SWEEP[:] = parse_sweep(args.sweep)
    if args.one_launch_rollout:
        if not args.route:
            ap.error("--one-launch-rollout is the route form's switch (the arm envs answer to KP1_FUSED_ROLLOUT)")
        os.environ["KP1_FUSED_ROUTE_ROLLOUT"] = "1"
    if args.train_tile:
        os.environ["KP1_TRAIN_TILE"] = "1"
    if args.rollout_form:
        if not (args.one_handle or args.single_seed):
            ap.error("--rollout-form selects the rollout of the --one-handle and --single-seed iterations (the other trainers have one form)")
        os.environ["KP1_ROLLOUT_RUN"] = "1" if args.rollout_form == "whole" else "0"
    if args.single_seed:
        if args.route or args.one_handle or args.dock or args.eval or args.route_eval or args.route_anchor or args.sweep:
            ap.error("--single-seed measures the single-seed Approach iteration on its own")
        args.ks = "1"
    if args.route and args.one_handle:
        ap.error("--one-handle is the Approach form; --route is always one handle")
    if args.eval and (args.route or args.dock or args.sweep):
        ap.error("--eval measures the Approach population's gate evaluation")
    if args.route_eval and (args.eval or args.route or args.dock or args.one_handle or args.sweep):
        ap.error("--route-eval measures the route population's final evaluations on its own")
    if args.route_anchor and (args.eval or args.route_eval or args.route or args.dock or args.one_handle or args.sweep):
        ap.error("--route-anchor measures the route population's teacher-anchor step on its own")
    if args.dock and (args.route or args.one_handle):
        ap.error("--dock measures the Finisher iteration in both forms")
    args.n_envs = args.n_envs or (12 if args.dock else 16)
    args.n_steps = args.n_steps or (256 if args.dock else 1024)
    if args.dock:
        return main_dock(args)
    if args.route_anchor:
        return main_route_anchor(args)
    if args.chain_form and not args.route_eval:
        ap.error("--chain-form belongs to --route-eval")
    if args.route_eval and args.chain_form:
        return main_route_chain_forms(args)
    if args.route_eval:
        return main_route_eval(args)
    if args.eval:
        return main_eval(args)
    args.ks = args.ks or ("1,2,4,8,16" if args.route or args.one_handle else "1,2,4,8")
    args.batch = args.batch or (512 if args.route else 256)
    rows = []
    for K in (int(k) for k in args.ks.split(",")):
        rows.append(measure(K, args))
        print(json.dumps(rows[-1]), flush=True)
    base = rows[0]["aggregate_env_steps_per_s"]
    for r in rows:
        r["aggregate_vs_first"] = r["aggregate_env_steps_per_s"] / base
    workload = (f"route_curriculum_prefix120_routeobs_sequence2 on synthetic_route.json (RoutePopulationPPO: one route env handle of K x {args.n_envs} envs)"
                if args.route else
                f"workspace_expansion_bigtrain.yaml Approach iteration (ApproachPopulationPPO: one env handle of K x {args.n_envs} envs)"
                if args.one_handle else
                f"workspace_expansion_bigtrain.yaml Approach iteration (PPO: the single-seed trainer, {args.n_envs} envs)"
                if args.single_seed else "workspace_expansion_bigtrain.yaml Approach iteration (PopulationPPO: one env handle per replica)")
    result = {"workload": f"{workload}, {args.n_envs} envs x {args.n_steps} steps per replica, "
                          f"minibatch {args.batch}, 2x{args.hidden}, curriculum on; seeds 7..7+K-1"
                          + (f"; sweep {dict(SWEEP)} (replica k takes value k % n)" if SWEEP else "")
                          + (f"; rollout form {args.rollout_form}" if args.rollout_form else "")
                          + ("; update form train tile" if args.train_tile else "") + ("; training monitor on" if args.monitor else ""), "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=2) + "\n")
    print(json.dumps({"aggregate_env_steps_per_s": {r["K"]: round(r["aggregate_env_steps_per_s"]) for r in rows}}))


def main_dock(args) -> None:
    import functools

    args.ks = args.ks or "1,2,4,8,16"
    args.batch = args.batch or 256
    cur = not args.no_curriculum
    rows = []
    for K in (int(k) for k in args.ks.split(",")):
        row = {"K": K}
        for form, build in (("one_handle", build_dock_one_handle), ("k_handles", build_dock_k_handles)):
            row[form] = measure(K, args, functools.partial(build, curriculum=cur))
        rows.append(row)
        print(json.dumps({"K": K, **{f: {k: round(v, 2) for k, v in row[f].items() if k.endswith("_ms")} for f in ("one_handle", "k_handles")}}), flush=True)
    for form in ("one_handle", "k_handles"):
        for r in rows:
            r[form]["rollout_vs_first"] = r[form]["rollout_ms"] / rows[0][form]["rollout_ms"]
    result = {"workload": f"dock_workspace_handoff_noop_ft_12env (golden handoff buffer), {args.n_envs} envs x {args.n_steps} steps per replica, "
                          f"minibatch {args.batch}, 2x{args.hidden}, graphs; "
                          + ("a 3-stage synthetic reverse curriculum (tools/population_bench.py DOCK_STAGES)" if cur else "no reverse curriculum")
                          + "; one_handle = DockPopulationPPO, k_handles = PopulationPPO with one handle per replica; seeds 7..7+K-1",
              "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=2) + "\n")
    print(json.dumps({f: {r["K"]: round(r[f]["rollout_ms"], 2) for r in rows} for f in ("one_handle", "k_handles")}))


if __name__ == "__main__":
    main()
