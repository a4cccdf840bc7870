#!/usr/bin/env python
"""Deterministic evaluation of 2x256 policies: the one-launch step (kp1_eval_step, one_launch=None) against the launch sequence per env step
(evaluate.run_episodes, one_launch=False), alternating in one process.

Policies: one 2x256 PPO on workspace_expansion_bigtrain after a few updates (evaluated through ppo.predict, i.e. on its training handle) and a
fresh 2x256 Finisher on dock_workspace_handoff_noop_ft_12env.  Workloads:
  (a) config4   workspace_coverage._run_pairs_columns on 8192 random-start pairs of workspace_full_coverage_randomstart_overnight, built as
                bench.py's config4_block builds them (Approach only)
  (b) gate      one gate evaluation: evaluate_workspace_expansion, 10 stages x 24 episodes, Approach -> Finisher, with handoff_confirm_steps
                2 and 0
Before any timing the two forms' results are compared: equal except the action-norm columns, which agree to 1e-13 relative.  Then one warm-up
of each form and --repeats timed runs of each, alternating, host clock around a device synchronise; median and max - min per form go to --out.

    python tools/eval_bench.py --out profiles/eval_step_h256.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/eval_bench.py --repeats 1 --out <dir>/eval_bench.json     (kernel durations)
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
from rl_brain_trainer_amd import workspace_coverage as wc  # noqa: E402
from rl_brain_trainer_amd.ppo import PPO, ActorCritic, InferencePolicy, PPOConfig  # noqa: E402
from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv  # noqa: E402

NORM_RTOL = 1e-13
FORMS = (("multi_launch", False), ("one_launch", None))


class StepCounter:
    """env steps of the episode runs an evaluation makes: per run the episodes' own steps (sum of step_count) and the lock-step count (its
    maximum = env-step launches of the one-launch form).  The tensors are reduced after the timed region."""

    def __init__(self) -> None:
        self.pending: list[torch.Tensor] = []
        self._orig = (ev.run_episodes, ev.run_episodes_fused)
        ev.run_episodes, ev.run_episodes_fused = self._wrap(ev.run_episodes), self._wrap(ev.run_episodes_fused)

    def _wrap(self, fn):
        def run(*a, **k):
            res, hand = fn(*a, **k)
            self.pending.append(res["step_count"])
            return res, hand

        return run

    def take(self) -> dict[str, int]:
        out = {"episode_env_steps": int(sum(int(t.sum()) for t in self.pending)), "lockstep_env_steps": int(sum(int(t.max()) for t in self.pending)),
               "episode_runs": len(self.pending)}
        self.pending = []
        return out


def columns_agree(got: torch.Tensor, ref: torch.Tensor) -> None:
    for k, name in enumerate(wc._COLS):
        if name.endswith("final_action_magnitude"):
            assert torch.allclose(got[:, k], ref[:, k], rtol=NORM_RTOL, atol=0.0), name
        else:
            assert torch.equal(got[:, k], ref[:, k]), name


def payloads_agree(a, b, path: str = "") -> None:
    if isinstance(b, dict):
        assert isinstance(a, dict) and a.keys() == b.keys(), path
        for k in b:
            payloads_agree(a[k], b[k], f"{path}/{k}")
    elif isinstance(b, list):
        assert isinstance(a, list) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            payloads_agree(x, y, f"{path}[{i}]")
    elif isinstance(b, float) and path.rsplit("/", 1)[-1] in ("final_action_magnitude", "mean_final_action_magnitude"):
        assert abs(a - b) <= NORM_RTOL * abs(b), (path, a, b)
    else:
        assert a == b, (path, a, b)


def timed(fn, counter: StepCounter) -> tuple[float, dict[str, int]]:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, counter.take()


def measure(name: str, run, agree, counter: StepCounter, repeats: int) -> dict:
    """run(one_launch) -> result; the forms alternate: agreement check (doubles as the warm-up of each form), then `repeats` timed pairs"""
    results = {form: run(flag) for form, flag in FORMS}
    agree(results["one_launch"], results["multi_launch"])
    counter.take()
    times: dict[str, list[float]] = {form: [] for form, _ in FORMS}
    steps: dict[str, dict[str, int]] = {}
    for _ in range(repeats):
        for form, flag in FORMS:
            dt, steps[form] = timed(lambda: run(flag), counter)
            times[form].append(dt)
    assert steps["one_launch"] == steps["multi_launch"], steps
    out = {"workload": name, "repeats": repeats, **steps["one_launch"]}
    for form, _ in FORMS:
        t = times[form]
        out[form] = {"median_s": statistics.median(t), "spread_s": max(t) - min(t), "seconds": t,
                     "episode_env_steps_per_s": steps[form]["episode_env_steps"] / statistics.median(t),
                     "us_per_lockstep_env_step": statistics.median(t) / steps[form]["lockstep_env_steps"] * 1e6}
    m, o = out["multi_launch"], out["one_launch"]
    out["speedup_median"] = m["median_s"] / o["median_s"]
    out["one_launch_wins"] = bool(m["median_s"] - o["median_s"] > m["spread_s"])    # the acceptance rule: by more than the old form's own spread
    print(f"[eval_bench] {name}: multi-launch {m['median_s'] * 1e3:.1f} ms (spread {m['spread_s'] * 1e3:.1f}), one-launch "
          f"{o['median_s'] * 1e3:.1f} ms (spread {o['spread_s'] * 1e3:.1f}), x{out['speedup_median']:.2f}, lock-step env steps "
          f"{out['lockstep_env_steps']}", file=sys.stderr, flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True, help="the JSON record")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=8192)
    ap.add_argument("--updates", type=int, default=3, help="PPO iterations before the Approach policy is evaluated")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py times device work: it needs the GPU")
    torch.cuda.set_device(args.device)
    dev = torch.device("cuda", args.device)
    cfg_dir = kcfg.builtin_config_dir()
    a_cfg = kcfg.to_env_config(kcfg.load_workspace_expansion_config(cfg_dir / "workspace_expansion_bigtrain.yaml"))
    dock = kcfg.load_yaml_file(cfg_dir / "dock_workspace_handoff_noop_ft_12env.yaml")
    dock["env"]["dock_reset"]["handoff_state_probability"] = 0.0      # the handoff-state buffer file is not shipped; the resets here are explicit anyway
    f_cfg = kcfg.to_env_config(dock)

    env = ArmKinematicVecEnv(a_cfg, 2048, device=args.device, seed=806)
    env.set_curriculum_stage(5)
    ppo = PPO(env, PPOConfig(n_steps=32, batch_size=8192, n_epochs=4, hidden=256, seed=806), backend="hip")
    for _ in range(args.updates):
        ppo.collect_rollouts()
        ppo.train()
    finisher = InferencePolicy(ActorCritic(256, dev, seed=2).state_dict(), device=dev)
    assert ev._is_fused_width(ev.policy_mlp(ppo.predict)) and ev._is_fused_width(ev.policy_mlp(finisher))
    counter = StepCounter()
    record = {"tool": "tools/eval_bench.py", "policies": "2x256 PPO (workspace_expansion_bigtrain, %d updates) through ppo.predict; fresh 2x256 Finisher" % args.updates,
              "timing": "host clock around a device synchronise; forms alternate in one process; one warm-up of each form first",
              "agreement": f"checked before timing: equal except the action-norm columns (rtol {NORM_RTOL})", "workloads": []}

    # (a) BASELINE configs[3] shard, as bench.py's config4_block builds it
    c4 = kcfg.to_env_config(kcfg.load_workspace_expansion_config(cfg_dir / "workspace_full_coverage_randomstart_overnight.yaml"))
    fk = wc._device_fk(args.device)
    targets, _ = wc.generate_workspace_target_map(c4, seed=940002, stage_samples_per_stage=96, random_samples=384, fk=fk)
    starts, _ = wc.generate_workspace_start_state_map(c4, seed=940003, stage_samples_per_stage=48, random_samples=384, fk=fk)
    n = args.pairs
    pairs, _ = wc.build_pair_sampler_summary(starts=starts, targets=targets, seed=940004, pair_count=n)
    common = dict(pairs=pairs[:n], first_env_id=3 * n, starts_by_id={r["start_id"]: r for r in starts}, targets_by_id={r["target_id"]: r for r in targets},
                  approach_policy=ppo.predict, approach_cfg=c4, finisher_policy=None, finisher_cfg=None, handoff_confirm_steps=2, device=args.device,
                  obs_stride=ppo.obs_w, seed=760001)
    record["workloads"].append(measure(f"config4: _run_pairs_columns, {n} pairs of workspace_full_coverage_randomstart_overnight",
                                       lambda flag: wc._run_pairs_columns(one_launch=flag, **common), columns_agree, counter, args.repeats))

    # (b) one gate evaluation
    for confirm in (2, 0):
        kw = dict(approach_policy=ppo.predict, finisher_policy=finisher, approach_cfg=a_cfg, finisher_cfg=f_cfg, episodes=24, seed=700001,
                  stage_indices=list(range(10)), handoff_confirm_steps=confirm, device=args.device, obs_stride=ppo.obs_w)
        record["workloads"].append(measure(f"gate: evaluate_workspace_expansion, 10 stages x 24 episodes, handoff_confirm_steps {confirm}",
                                           lambda flag: ev.evaluate_workspace_expansion(one_launch=flag, **kw), payloads_agree, counter, args.repeats))
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=2) + "\n")
    print(json.dumps({"out": str(out), "wins": {w["workload"].split(",")[0] + w["workload"][-2:]: w["one_launch_wins"]
                                                  for w in record["workloads"]}}))
    env.close()


if __name__ == "__main__":
    main()
