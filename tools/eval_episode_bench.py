#!/usr/bin/env python
"""Deterministic evaluation of 2x256 policies: all env steps of a phase in one launch (kp1_eval_episodes, whole_episodes=True) against one
launch per env step (kp1_eval_step, whole_episodes=False: the code path of evaluate.run_episodes_fused as it was before the keyword
existed), alternating in one process.  A sibling of tools/eval_bench.py with its policies and workloads, plus a dock evaluation:
  (a) config4   workspace_coverage._run_pairs_columns on 8192 random-start pairs of workspace_full_coverage_randomstart_overnight, built as
                bench.py's config4_block builds them (Approach only)
  (b) gate      one gate evaluation: evaluate_workspace_expansion, 10 stages x 24 episodes, Approach -> Finisher, with handoff_confirm_steps
                2 and 0
  (c) dock      train_dock.evaluate_dock, 512 episodes of dock_workspace_handoff_noop_ft_12env (its default --eval-episodes)
Before any timing the two forms' results are asserted EQUAL (both run the same action norm and bookkeeping: no tolerance).  Then one warm-up
of each form and --repeats timed runs of each, alternating, host clock around a device synchronise; median and max - min per form go to
--out.  ``whole_episodes_wins`` is the acceptance rule that sets evaluate.WHOLE_EPISODES_DEFAULT: the whole-episode median beats the
per-step median by more than the per-step form's own spread.

    python tools/eval_episode_bench.py --out profiles/eval_episodes.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from rl_brain_trainer_amd import config as kcfg  # noqa: E402
from rl_brain_trainer_amd import evaluate as ev  # noqa: E402
from rl_brain_trainer_amd import train_dock  # noqa: E402
from rl_brain_trainer_amd import workspace_coverage as wc  # noqa: E402
from rl_brain_trainer_amd.ppo import PPO, ActorCritic, InferencePolicy, PPOConfig  # noqa: E402
from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv  # noqa: E402

FORMS = (("per_step", False), ("whole_episodes", True))


class StepCounter:
    """env steps of the episode runs an evaluation makes: per run the episodes' own steps (sum of step_count) and the lock-step count (its
    maximum = launches of the per-step form).  The tensors are reduced after the timed region."""

    def __init__(self) -> None:
        self.pending: list[torch.Tensor] = []
        fn = ev.run_episodes_fused

        def run(*a, **k):
            res, hand = fn(*a, **k)
            self.pending.append(res["step_count"])
            return res, hand

        ev.run_episodes_fused = run

    def take(self) -> dict[str, int]:
        out = {"episode_env_steps": int(sum(int(t.sum()) for t in self.pending)), "lockstep_env_steps": int(sum(int(t.max()) for t in self.pending)),
               "episode_runs": len(self.pending)}
        self.pending = []
        return out


def equal(a, b) -> None:
    assert torch.equal(a, b) if isinstance(b, torch.Tensor) else a == b


def timed(fn, counter: StepCounter) -> tuple[float, dict[str, int]]:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, counter.take()


def measure(name: str, entry: str, run, counter: StepCounter, repeats: int) -> dict:
    """run(whole_episodes) -> result; the forms alternate: equality check (doubles as the warm-up of each form), then `repeats` timed pairs"""
    results = {form: run(flag) for form, flag in FORMS}
    equal(results["whole_episodes"], results["per_step"])
    counter.take()
    times: dict[str, list[float]] = {form: [] for form, _ in FORMS}
    steps: dict[str, dict[str, int]] = {}
    for _ in range(repeats):
        for form, flag in FORMS:
            dt, steps[form] = timed(lambda: run(flag), counter)
            times[form].append(dt)
    assert steps["whole_episodes"] == steps["per_step"], steps
    out = {"workload": name, "entry_point": entry, "repeats": repeats, **steps["per_step"]}
    for form, _ in FORMS:
        t = times[form]
        out[form] = {"median_s": statistics.median(t), "spread_s": max(t) - min(t), "seconds": t,
                     "episode_env_steps_per_s": steps[form]["episode_env_steps"] / statistics.median(t),
                     "us_per_lockstep_env_step": statistics.median(t) / steps[form]["lockstep_env_steps"] * 1e6}
    p, w = out["per_step"], out["whole_episodes"]
    out["speedup_median"] = p["median_s"] / w["median_s"]
    out["whole_episodes_wins"] = bool(p["median_s"] - w["median_s"] > p["spread_s"])    # the acceptance rule: by more than the old form's own spread
    print(f"[eval_episode_bench] {name}: per-step {p['median_s'] * 1e3:.1f} ms (spread {p['spread_s'] * 1e3:.1f}), whole-episode "
          f"{w['median_s'] * 1e3:.1f} ms (spread {w['spread_s'] * 1e3:.1f}), x{out['speedup_median']:.2f}, lock-step env steps "
          f"{out['lockstep_env_steps']}", file=sys.stderr, flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True, help="the JSON record")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=8192)
    ap.add_argument("--dock-episodes", type=int, default=512)
    ap.add_argument("--updates", type=int, default=3, help="PPO iterations before the Approach policy is evaluated")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_episode_bench.py times device work: it needs the GPU")
    torch.cuda.set_device(args.device)
    dev = torch.device("cuda", args.device)
    cfg_dir = kcfg.builtin_config_dir()
    a_cfg = kcfg.to_env_config(kcfg.load_workspace_expansion_config(cfg_dir / "workspace_expansion_bigtrain.yaml"))
    dock = kcfg.load_yaml_file(cfg_dir / "dock_workspace_handoff_noop_ft_12env.yaml")
    dock["env"]["dock_reset"]["handoff_state_probability"] = 0.0      # the handoff-state buffer file is not shipped
    f_cfg = kcfg.to_env_config(dock)

    env = ArmKinematicVecEnv(a_cfg, 2048, device=args.device, seed=806)
    env.set_curriculum_stage(5)
    ppo = PPO(env, PPOConfig(n_steps=32, batch_size=8192, n_epochs=4, hidden=256, seed=806), backend="hip")
    for _ in range(args.updates):
        ppo.collect_rollouts()
        ppo.train()
    finisher = InferencePolicy(ActorCritic(256, dev, seed=2).state_dict(), device=dev)
    denv = ArmKinematicVecEnv(f_cfg, 64, device=args.device, seed=11)
    dock_ppo = PPO(denv, PPOConfig(n_steps=4, batch_size=256, n_epochs=1, hidden=256, seed=11), backend="hip")
    assert all(ev._is_fused_width(ev.policy_mlp(p)) for p in (ppo.predict, finisher, dock_ppo.predict))
    counter = StepCounter()
    record = {"tool": "tools/eval_episode_bench.py",
              "policies": "2x256 PPO (workspace_expansion_bigtrain, %d updates) through ppo.predict; fresh 2x256 Finisher; fresh 2x256 dock PPO" % args.updates,
              "timing": "host clock around a device synchronise; forms alternate in one process; one warm-up of each form first",
              "agreement": "asserted before timing: the two forms' results are equal", "workloads": []}

    c4 = kcfg.to_env_config(kcfg.load_workspace_expansion_config(cfg_dir / "workspace_full_coverage_randomstart_overnight.yaml"))
    fk = wc._device_fk(args.device)
    targets, _ = wc.generate_workspace_target_map(c4, seed=940002, stage_samples_per_stage=96, random_samples=384, fk=fk)
    starts, _ = wc.generate_workspace_start_state_map(c4, seed=940003, stage_samples_per_stage=48, random_samples=384, fk=fk)
    n = args.pairs
    pairs, _ = wc.build_pair_sampler_summary(starts=starts, targets=targets, seed=940004, pair_count=n)
    common = dict(pairs=pairs[:n], first_env_id=3 * n, starts_by_id={r["start_id"]: r for r in starts}, targets_by_id={r["target_id"]: r for r in targets},
                  approach_policy=ppo.predict, approach_cfg=c4, finisher_policy=None, finisher_cfg=None, handoff_confirm_steps=2, device=args.device,
                  obs_stride=ppo.obs_w, seed=760001)
    record["workloads"].append(measure(f"config4: _run_pairs_columns, {n} pairs of workspace_full_coverage_randomstart_overnight", "run_pairs",
                                       lambda flag: wc._run_pairs_columns(whole_episodes=flag, **common), counter, args.repeats))
    for confirm in (2, 0):
        kw = dict(approach_policy=ppo.predict, finisher_policy=finisher, approach_cfg=a_cfg, finisher_cfg=f_cfg, episodes=24, seed=700001,
                  stage_indices=list(range(10)), handoff_confirm_steps=confirm, device=args.device, obs_stride=ppo.obs_w)
        record["workloads"].append(measure(f"gate: evaluate_workspace_expansion, 10 stages x 24 episodes, handoff_confirm_steps {confirm}",
                                           "evaluate_workspace_expansion",
                                           lambda flag: ev.evaluate_workspace_expansion(whole_episodes=flag, **kw), counter, args.repeats))
    record["workloads"].append(measure(f"dock: evaluate_dock, {args.dock_episodes} episodes of dock_workspace_handoff_noop_ft_12env", "evaluate_dock",
                                       lambda flag: train_dock.evaluate_dock(dock_ppo, f_cfg, episodes=args.dock_episodes, seed=10_011, device=args.device,
                                                                             whole_episodes=flag), counter, args.repeats))
    record["defaults_by_the_rule"] = {e: all(w["whole_episodes_wins"] for w in record["workloads"] if w["entry_point"] == e)
                                      for e in sorted({w["entry_point"] for w in record["workloads"]})}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=2) + "\n")
    print(json.dumps({"out": str(out), "defaults_by_the_rule": record["defaults_by_the_rule"]}))
    env.close()
    denv.close()


if __name__ == "__main__":
    main()
