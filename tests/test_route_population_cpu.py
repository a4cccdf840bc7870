"""Route-curriculum population without a GPU: the population ABI is exported, --seeds / --seed exclude each other on train_route, and
RoutePopulationPPO refuses what it does not support before touching a device."""
from __future__ import annotations

import ctypes as C
import io
import zipfile

import pytest

from rl_brain_trainer_amd import native
from rl_brain_trainer_amd.ppo import PPOConfig


def test_route_population_symbols_exported():
    lib = C.CDLL(str(native.LIB_PATH))
    declared = native.declared_symbols()
    for name in ("kp1_seed_blocks", "kp1_route_create_population", "kp1_route_num_replicas", "kp1_route_set_replica_window",
                 "kp1_route_curriculum_create_population", "kp1_route_curriculum_observe_population", "kp1_route_curriculum_read_replica"):
        assert hasattr(lib, name), name
        assert name in declared, name
    lib.kp1_route_num_replicas.argtypes = [C.c_void_p]
    assert lib.kp1_route_num_replicas(None) == 0
    header = (native.PKG_DIR.parent / "include" / "kp1_route.h").read_text()
    assert "#define KP1_ROUTE_MAX_REPLICAS 16" in header


def test_route_population_classes_exported():
    from rl_brain_trainer_amd.population import PopulationPPO, RoutePopulationPPO
    from rl_brain_trainer_amd.route_curriculum import RoutePrefixCurriculumDevice, RoutePrefixCurriculumPopulation
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv, RouteVecEnv

    assert issubclass(RoutePopulationPPO, PopulationPPO)
    assert issubclass(RoutePopulationVecEnv, RouteVecEnv)
    assert issubclass(RoutePrefixCurriculumPopulation, RoutePrefixCurriculumDevice)
    assert RoutePrefixCurriculumPopulation.needs_episode_records is False


def test_train_route_seeds_and_seed_exclude_each_other(capsys):
    from rl_brain_trainer_amd import train_route

    parser = train_route.build_arg_parser()
    args = parser.parse_args(["--config", "c.yaml", "--seeds", "7,8,9,10"])
    assert args.seeds == "7,8,9,10" and args.seed is None
    assert parser.parse_args(["--config", "c.yaml", "--seed", "7"]).seeds is None
    with pytest.raises(SystemExit):
        parser.parse_args(["--config", "c.yaml", "--seed", "7", "--seeds", "7,8"])
    assert "not allowed with argument" in capsys.readouterr().err


class _EnabledDist:
    enabled, world_size, rank = True, 2, 0


@pytest.mark.parametrize("seeds, cfg, kwargs, match", [
    ([7, 8], PPOConfig(hidden=256), {}, "hidden=256"),
    ([7, 7], PPOConfig(hidden=64), {}, "distinct"),
    (list(range(17)), PPOConfig(hidden=64), {}, "at most 16"),
    ([7, 8], PPOConfig(hidden=64), {"teacher_anchor": object()}, "teacher-anchor"),
    ([7, 8], PPOConfig(hidden=64), {"dist": _EnabledDist()}, "data parallel"),
])
def test_route_population_refusals(seeds, cfg, kwargs, match):
    from rl_brain_trainer_amd.population import RoutePopulationPPO

    with pytest.raises(ValueError, match=match):
        RoutePopulationPPO(seeds, cfg, None, **kwargs)


def test_route_population_refuses_other_envs():
    from rl_brain_trainer_amd.population import RoutePopulationPPO

    with pytest.raises(TypeError, match="RoutePopulationVecEnv"):
        RoutePopulationPPO([7, 8], PPOConfig(hidden=64), object())


def _write_checkpoint(path, actor_extra_steps: int) -> None:
    """a checkpoint zip with a 2x64 route policy and an Adam state whose actor tensors took `actor_extra_steps` more steps"""
    import torch

    from rl_brain_trainer_amd import checkpoint
    from rl_brain_trainer_amd.ppo import ActorCritic

    pol = ActorCritic(64, torch.device("cpu"), obs_dim=80)
    state = {}
    for i, (name, shape) in enumerate(pol.spec):
        actor = name.startswith(("mlp_extractor.policy_net", "action_net"))
        state[i] = {"step": torch.tensor(float(10 + (actor_extra_steps if actor else 0))), "exp_avg": torch.zeros(shape), "exp_avg_sq": torch.zeros(shape)}
    opt = {"state": state, "param_groups": [{"params": list(range(len(pol.spec)))}]}
    buf_p, buf_o = io.BytesIO(), io.BytesIO()
    torch.save(pol.state_dict(), buf_p)
    torch.save(opt, buf_o)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", buf_p.getvalue())
        z.writestr("policy.optimizer.pth", buf_o.getvalue())
    assert checkpoint.load_optimizer_state_dict(path)["state"][0]["step"] == 10.0


def test_route_population_refuses_actor_extra_steps_checkpoint(tmp_path):
    from rl_brain_trainer_amd.population import RoutePopulationPPO

    good, bad = tmp_path / "good.zip", tmp_path / "anchored.zip"
    _write_checkpoint(good, 0)
    _write_checkpoint(bad, 3)
    RoutePopulationPPO.check_init_checkpoint(str(good))
    with pytest.raises(ValueError, match="actor_extra_steps"):
        RoutePopulationPPO.check_init_checkpoint(str(bad))


def _route_yaml(tmp_path, anchor: bool) -> str:
    import json

    import yaml

    from conftest import GOLDEN

    cfgd = json.loads((GOLDEN / "configs" / "route_curriculum_prefix120_routeobs_sequence2.json").read_text())
    cfgd["route"]["route_path"] = str(GOLDEN / "synthetic_route.json")
    cfgd["route"].pop("init_checkpoint", None)
    cfgd["route"]["teacher_anchor"] = {"enabled": anchor, "dataset_path": str(tmp_path / "none.npz")}
    path = tmp_path / "route.yaml"
    path.write_text(yaml.safe_dump(cfgd))
    return str(path)


@pytest.mark.parametrize("extra, match", [
    ([], "--hidden 64 or 128"),
    (["--hidden", "256"], "--hidden 64 or 128"),
])
def test_train_route_seeds_refuses_hidden_256(tmp_path, monkeypatch, extra, match):
    from rl_brain_trainer_amd import train_route

    monkeypatch.setattr("torch.cuda.set_device", lambda *_: None)
    with pytest.raises(ValueError, match=match):
        train_route.main(["--config", _route_yaml(tmp_path, False), "--output-dir", str(tmp_path / "o"), "--seeds", "7,8"] + extra)


def test_train_route_seeds_refuses_teacher_anchor(tmp_path, monkeypatch):
    from rl_brain_trainer_amd import train_route

    monkeypatch.setattr("torch.cuda.set_device", lambda *_: None)
    with pytest.raises(ValueError, match="teacher-anchor"):
        train_route.main(["--config", _route_yaml(tmp_path, True), "--output-dir", str(tmp_path / "o"), "--seeds", "7,8", "--hidden", "64"])
