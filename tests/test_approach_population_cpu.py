"""Approach population on one env handle, without a GPU: the population env / tracker ABI is exported and declared, the classes exist, and
everything that is refused is refused before any device work."""
from __future__ import annotations

import ctypes as C

import pytest

from rl_brain_trainer_amd import native
from rl_brain_trainer_amd.ppo import PPOConfig

NEW_SYMBOLS = ("kp1_curriculum_create_population", "kp1_curriculum_observe_population", "kp1_curriculum_read_replica",
               "kp1_bind_population_stages")


def test_approach_population_symbols_exported_and_declared():
    lib = C.CDLL(str(native.LIB_PATH))
    declared = native.declared_symbols()
    for name in NEW_SYMBOLS + ("kp1_seed_blocks",):
        assert hasattr(lib, name), name
        assert name in declared, name
    header = (native.PKG_DIR.parent / "include" / "kp1_ppo.h").read_text()
    assert "#define KP1_CURRICULUM_MAX_REPLICAS 16" in header
    lib.kp1_abi_version.restype = C.c_int
    assert lib.kp1_abi_version() == 1


def test_approach_population_host_checks_in_the_library():
    """argument checks of the new entry points that fail before the device is touched"""
    lib = C.CDLL(str(native.LIB_PATH))
    vp, i32 = C.c_void_p, C.c_int32
    lib.kp1_bind_population_stages.argtypes = [vp, vp, i32]
    lib.kp1_curriculum_read_replica.argtypes = [i32, vp, i32, i32, vp, vp]
    lib.kp1_curriculum_observe_population.argtypes = [i32, vp, vp, i32, i32, i32, vp]
    lib.kp1_curriculum_create_population.argtypes = [i32, i32, C.c_double, i32, i32, i32, vp, C.POINTER(vp)]
    out = vp()
    stages = (i32 * 17)()
    assert lib.kp1_bind_population_stages(None, None, 0) != native.KP1_OK
    assert lib.kp1_curriculum_create_population(0, 17, 0.5, 4, 4, 3, C.cast(stages, vp), C.byref(out)) != native.KP1_OK
    assert lib.kp1_curriculum_create_population(0, 0, 0.5, 4, 4, 3, C.cast(stages, vp), C.byref(out)) != native.KP1_OK
    assert not out.value
    buf = (C.c_uint8 * 64)()
    assert lib.kp1_curriculum_observe_population(0, None, C.cast(buf, vp), 16, 2, 16, None) != native.KP1_OK
    assert lib.kp1_curriculum_observe_population(0, C.cast(buf, vp), C.cast(buf, vp), 16, 17, 16, None) != native.KP1_OK
    assert lib.kp1_curriculum_read_replica(0, C.cast(buf, vp), 2, 2, C.cast(buf, vp), None) != native.KP1_OK
    assert lib.kp1_curriculum_read_replica(0, C.cast(buf, vp), 2, -1, C.cast(buf, vp), None) != native.KP1_OK


def test_approach_population_classes_exported():
    from rl_brain_trainer_amd.curriculum import PointCurriculum, PointCurriculumPopulation
    from rl_brain_trainer_amd.population import ApproachPopulationPPO, OneHandlePopulationPPO, PopulationPPO, RoutePopulationPPO
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    assert issubclass(ArmKinematicPopulationVecEnv, ArmKinematicVecEnv) and ArmKinematicPopulationVecEnv.is_population
    assert issubclass(PointCurriculumPopulation, PointCurriculum)
    assert issubclass(ApproachPopulationPPO, OneHandlePopulationPPO) and issubclass(RoutePopulationPPO, OneHandlePopulationPPO)
    assert issubclass(OneHandlePopulationPPO, PopulationPPO)
    for name in ("_reset_envs", "_policy_env_step", "_curriculum_observe", "_warm_curricula"):
        assert name in OneHandlePopulationPPO.__dict__, name


def _env_cfg(mode: str = "approach"):
    from rl_brain_trainer_amd import config as kcfg

    if mode == "dock":
        return kcfg.to_env_config(kcfg.load_yaml_file(kcfg.builtin_config_dir() / "dock_workspace_handoff_noop_ft_12env.yaml"))
    return kcfg.to_env_config(kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"))


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to create a device handle fails the test: the refusals below must come first"""
    import torch

    def touched(*_a, **_k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(torch.cuda, "is_available", touched)
    monkeypatch.setattr(native, "load", touched)


@pytest.mark.parametrize("seeds, mode, kwargs, match", [
    (list(range(17)), "approach", {}, "at most 16"),
    ([7, 7], "approach", {}, "distinct"),
    ([], "approach", {}, "at least one"),
    ([7, 8], "dock", {}, "dock-mode"),
    ([7, 8], "approach", {"real": "f64"}, "f32"),
])
def test_population_env_refusals(no_device, seeds, mode, kwargs, match):
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    with pytest.raises(ValueError, match=match):
        ArmKinematicPopulationVecEnv(_env_cfg(mode), seeds, 16, **kwargs)


def test_population_tracker_refuses_more_than_16_replicas(no_device):
    from rl_brain_trainer_amd.curriculum import PointCurriculumPopulation

    with pytest.raises(ValueError, match="1 to 16"):
        PointCurriculumPopulation(success_rate_threshold=0.5, window_episodes=4, min_episodes_per_stage=4, max_stage_index=3,
                                  initial_stage_indices=[0] * 17)


def _bare(cls, **attrs):
    """an instance that never ran __init__ (no device handle behind it)"""
    obj = cls.__new__(cls)
    obj.__dict__.update(attrs)
    return obj


class _PlainEnv:
    n_envs = 48


def test_population_tracker_refuses_env_count_not_a_multiple_of_k(no_device):
    from rl_brain_trainer_amd.curriculum import PointCurriculumPopulation
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    cur = _bare(PointCurriculumPopulation, K=3)
    env = _bare(ArmKinematicPopulationVecEnv, n_envs=32, K=3)
    with pytest.raises(ValueError, match="does not split"):
        cur.attach(env)
    with pytest.raises(TypeError, match="ArmKinematicPopulationVecEnv"):
        cur.attach(_PlainEnv())


def test_population_tracker_has_no_chunk_form(no_device):
    import torch

    from rl_brain_trainer_amd.curriculum import PointCurriculumPopulation

    cur = _bare(PointCurriculumPopulation, K=2)
    with pytest.raises(TypeError, match="no data-parallel form"):
        cur.observe_chunk(torch.zeros(64, dtype=torch.uint8), 16, 2, 2)
    with pytest.raises(TypeError):
        cur.stage_ptr


def test_plain_ppo_refuses_a_population_env(no_device):
    from rl_brain_trainer_amd.ppo import PPO
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    env = _bare(ArmKinematicPopulationVecEnv, n_envs=32, K=2)
    with pytest.raises(TypeError, match="population"):
        PPO(env, PPOConfig(hidden=64))


class _EnabledDist:
    enabled, world_size, rank = True, 2, 0


@pytest.mark.parametrize("seeds, cfg, kwargs, match", [
    ([7, 8], PPOConfig(hidden=256), {}, "hidden=256"),
    ([7, 7], PPOConfig(hidden=64), {}, "distinct"),
    (list(range(17)), PPOConfig(hidden=64), {}, "at most 16"),
    ([7, 8], PPOConfig(hidden=64), {"teacher_anchor": object()}, "teacher-anchor"),
    ([7, 8], PPOConfig(hidden=64), {"dist": _EnabledDist()}, "data parallel"),
])
def test_approach_population_ppo_refusals(no_device, seeds, cfg, kwargs, match):
    from rl_brain_trainer_amd.population import ApproachPopulationPPO

    with pytest.raises(ValueError, match=match):
        ApproachPopulationPPO(seeds, cfg, None, **kwargs)


def test_approach_population_ppo_refuses_other_envs_and_trackers(no_device):
    from rl_brain_trainer_amd.curriculum import PointCurriculum
    from rl_brain_trainer_amd.population import ApproachPopulationPPO
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    with pytest.raises(TypeError, match="ArmKinematicPopulationVecEnv"):
        ApproachPopulationPPO([7, 8], PPOConfig(hidden=64), _bare(ArmKinematicVecEnv, n_envs=16))
    env = _bare(ArmKinematicPopulationVecEnv, seeds=[7, 8], K=2, n_envs=32)
    with pytest.raises(ValueError, match="made for seeds"):
        ApproachPopulationPPO([7, 9], PPOConfig(hidden=64), env)
    with pytest.raises(TypeError, match="PointCurriculumPopulation"):
        ApproachPopulationPPO([7, 8], PPOConfig(hidden=64), env, curriculum=_bare(PointCurriculum))


def test_train_seeds_refuses_hidden_256_before_device_work(tmp_path, monkeypatch, no_device):
    import yaml

    from rl_brain_trainer_amd import config as kcfg
    from rl_brain_trainer_amd import train

    monkeypatch.setattr("torch.cuda.set_device", lambda *_: None)
    overlay = {"base_config": str(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"),
               "workspace_expansion": {"init_approach_checkpoint": "", "finisher_checkpoint": ""}}
    cfg_path = tmp_path / "run.yaml"
    cfg_path.write_text(yaml.safe_dump(overlay))
    with pytest.raises(ValueError, match="hidden=256"):
        train.main(["--config", str(cfg_path), "--artifact-root", str(tmp_path / "o"), "--seeds", "7,8", "--hidden", "256"])
