"""Per-replica PPO hyper-parameters on the host (no GPU): --sweep parsing and replica order, the refusals of overrides and of --sweep, replica
directory names, population_summary fields, and train.py --seeds --resume-from refusing before any device work."""
from __future__ import annotations

import pytest
import torch

from rl_brain_trainer_amd import native
from rl_brain_trainer_amd.ppo import PPOConfig


@pytest.fixture
def no_device(monkeypatch):
    def touched(*_a, **_k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(torch.cuda, "is_available", touched)
    monkeypatch.setattr(native, "load", touched)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)


def test_header_declares_the_sweep_entry_points():
    assert {"kp1_mlp_set_replica_hparams", "kp1_gae_scan_replicas"} <= set(native.declared_symbols())


def test_sweep_order_is_seed_major_cartesian():
    from rl_brain_trainer_amd.population import plan_replicas

    seeds, overrides, names = plan_replicas("7,8", ["learning_rate=1e-4,3e-4", "gamma=0.99,0.95"])
    assert seeds == [7, 7, 7, 7, 8, 8, 8, 8]
    assert overrides[:4] == [{"learning_rate": 1e-4, "gamma": 0.99}, {"learning_rate": 1e-4, "gamma": 0.95},
                             {"learning_rate": 3e-4, "gamma": 0.99}, {"learning_rate": 3e-4, "gamma": 0.95}]
    assert overrides[4:] == overrides[:4]
    assert names[0] == "seed_7_learning_rate_0.0001_gamma_0.99" and names[-1] == "seed_8_learning_rate_0.0003_gamma_0.95"
    assert len(set(names)) == len(names)


def test_without_sweep_nothing_changes():
    from rl_brain_trainer_amd.population import plan_replicas

    assert plan_replicas("7,8,9", None) == ([7, 8, 9], None, ["seed_7", "seed_8", "seed_9"])
    with pytest.raises(ValueError, match="distinct"):
        plan_replicas("7,7", None)


@pytest.mark.parametrize("spec, match", [
    (["momentum=0.9"], "unknown key"),
    (["n_steps=64,128"], "geometry"),
    (["batch_size=64"], "geometry"),
    (["hidden=64"], "geometry"),
    (["seed=1,2"], "seed"),
    (["learning_rate"], "KEY=v1"),
    (["learning_rate=abc"], "numbers"),
    (["learning_rate="], "at least one"),
    (["learning_rate=nan"], "finite"),
    (["learning_rate=1e-4", "learning_rate=3e-4"], "twice"),
    (["learning_rate=1e-4,1e-4"], "distinct"),
    (["learning_rate=" + ",".join(str(1e-5 * (i + 1)) for i in range(9))], "at most 16"),
])
def test_sweep_refusals(spec, match):
    from rl_brain_trainer_amd.population import plan_replicas

    with pytest.raises(ValueError, match=match):
        plan_replicas("7,8", spec)


def test_sweep_needs_seeds():
    from rl_brain_trainer_amd.population import plan_replicas

    with pytest.raises(ValueError, match="needs --seeds"):
        plan_replicas(None, ["learning_rate=1e-4"])


@pytest.mark.parametrize("module", ["train", "train_dock", "train_route"])
def test_trainers_refuse_sweep_without_seeds(no_device, module):
    import importlib

    mod = importlib.import_module(f"rl_brain_trainer_amd.{module}")
    with pytest.raises(ValueError, match="needs --seeds"):
        mod.main(["--config", "unused.yaml", "--seed", "3", "--sweep", "learning_rate=1e-4"])


@pytest.mark.parametrize("overrides, match", [
    ([{"n_epochs": 4}, {}], "geometry"),
    ([{"normalize_advantage": 0.0}, {}], "geometry"),
    ([{"seed": 3}, {}], "seed"),
    ([{"lr": 1e-4}, {}], "unknown override"),
    ([{"learning_rate": "fast"}, {}], "not a number"),
    ([{"learning_rate": float("inf")}, {}], "not finite"),
    ([{}], "one per replica"),
])
def test_override_refusals(overrides, match):
    from rl_brain_trainer_amd.population import PopulationPPO

    def unused(_seed):
        raise AssertionError("the env factory must not be called for a refused configuration")

    with pytest.raises(ValueError, match=match):
        PopulationPPO([7, 8], PPOConfig(), unused, overrides=overrides)


def test_repeated_seeds_with_distinct_overrides_pass_the_host_checks():
    from rl_brain_trainer_amd.population import PopulationPPO, check_overrides

    out = check_overrides([7, 7, 8], [{"learning_rate": 1e-4}, {"learning_rate": 3e-4}, {}])
    assert out == [{"learning_rate": 1e-4}, {"learning_rate": 3e-4}, {}]
    seeds, _dist, ov = PopulationPPO._check_population_args([7, 7], PPOConfig(), None, None, [{"gamma": 0.9}, {"gamma": 0.95}])
    assert seeds == [7, 7] and ov == [{"gamma": 0.9}, {"gamma": 0.95}]
    with pytest.raises(ValueError, match=r"\(seed, overrides\) pairs must be distinct"):
        check_overrides([7, 7], [{"gamma": 0.9}, {"gamma": 0.9}])


def test_population_env_takes_repeated_seeds_on_request(no_device):
    from rl_brain_trainer_amd import config as kcfg
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    env_cfg = kcfg.to_env_config(kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"))
    with pytest.raises(ValueError, match="distinct"):
        ArmKinematicPopulationVecEnv(env_cfg, [7, 7], 16)
    with pytest.raises(AssertionError, match="device work"):     # past the host checks: the handle is about to be created
        ArmKinematicPopulationVecEnv(env_cfg, [7, 7], 16, repeated_seeds=True)


def test_population_summary_fields():
    from rl_brain_trainer_amd.population import population_summary

    class Pop:
        seeds, K, num_timesteps = [7, 7], 2, 100
        overrides = [{"learning_rate": 1e-4}, {"learning_rate": 3e-4}]

    rows = [{"seed": 7, "best_score": 0.2}, {"seed": 7, "best_score": 0.5}]
    out = population_summary(Pop(), rows, wall_seconds=1.0, selection="score")
    assert [r["replica"] for r in out["per_seed"]] == ["seed_7_learning_rate_0.0001", "seed_7_learning_rate_0.0003"]
    assert [r["overrides"] for r in out["per_seed"]] == Pop.overrides
    assert out["best_seed"] == 7 and out["best_overrides"] == {"learning_rate": 3e-4}
    plain = population_summary(type("P", (), {"seeds": [7, 8], "K": 2, "num_timesteps": 1, "overrides": [{}, {}]})(),
                               [{"seed": 7, "best_score": None}, {"seed": 8, "best_score": None}], wall_seconds=1.0, selection="s")
    assert [r["replica"] for r in plain["per_seed"]] == ["seed_7", "seed_8"] and plain["best_overrides"] is None


# ---------------------------------------------------------------------------------------------------------------- train.py --seeds resume
def _save_zip(path, hidden=64, adam_extra=0):
    """a minimal SB3-style archive: policy + optimizer state (what check_init_checkpoint reads)"""
    from types import SimpleNamespace

    from rl_brain_trainer_amd import checkpoint
    from rl_brain_trainer_amd.ppo import ActorCritic, PPOConfig

    pol = ActorCritic(hidden, torch.device("cpu"), seed=1)
    n = pol.numel
    fake = SimpleNamespace(cfg=PPOConfig(hidden=hidden), policy=pol, adam_m=torch.zeros(n), adam_v=torch.zeros(n), adam_t=3,
                           actor_extra_steps=adam_extra, num_timesteps=1000, n_train_calls=1, obs_dim=56, obs_w=64, n_envs=16, seed=1,
                           curriculum=None, env=None, dist=SimpleNamespace(world_size=1), backend="hip", device=torch.device("cpu"))
    return checkpoint.save(path, fake, None)


def _train_args(tmp_path):
    import yaml

    from rl_brain_trainer_amd import config as kcfg

    cfg_path = tmp_path / "run.yaml"
    cfg_path.write_text(yaml.safe_dump({"base_config": str(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"),
                                        "workspace_expansion": {"init_approach_checkpoint": "", "finisher_checkpoint": ""}}))
    return ["--config", str(cfg_path), "--n-envs", "16", "--n-steps", "64", "--batch-size", "256", "--hidden", "64", "--log-every", "0",
            "--artifact-root", str(tmp_path / "out")]


def test_train_seeds_resume_refusals_come_first(tmp_path, no_device):
    from rl_brain_trainer_amd import train

    common = _train_args(tmp_path)
    anchored = _save_zip(tmp_path / "anchored", adam_extra=2)
    wide = _save_zip(tmp_path / "wide", hidden=256)
    with pytest.raises(ValueError, match="teacher-anchor"):
        train.main(common + ["--seeds", "3,4", "--resume-from", str(anchored)])
    with pytest.raises(ValueError, match="2x256"):
        train.main(common + ["--seeds", "3,4", "--resume-from", str(wide)])
    root = tmp_path / "earlier"
    (root / "seed_3").mkdir(parents=True)
    with pytest.raises(ValueError, match=r"seeds \[3, 4\]"):
        train.main(common + ["--seeds", "3,4", "--resume-from", str(root)])


def test_train_seeds_resume_no_longer_refused(tmp_path, no_device):
    """the parent refused train.py --seeds with a checkpoint; now it gets past every host check to the device work"""
    from rl_brain_trainer_amd import train

    common = _train_args(tmp_path)
    ok = _save_zip(tmp_path / "ok")
    with pytest.raises(AssertionError, match="device work"):
        train.main(common + ["--seeds", "3,4", "--resume-from", str(ok)])
