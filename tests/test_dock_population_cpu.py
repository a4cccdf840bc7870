"""Dock (Finisher) population without a GPU: the dock population ABI is exported, the ctypes tracker layouts match the header, and
`train_dock --seeds --resume-from` resolves its checkpoints -- a zip for every seed, or seed_<s>/model_latest.zip of an earlier --seeds
root -- and refuses what a population cannot resume, all before any device work."""
from __future__ import annotations

import ctypes as C
import io
import json
import re
import zipfile

import pytest

from rl_brain_trainer_amd import native


def test_dock_population_symbols_exported():
    lib = C.CDLL(str(native.LIB_PATH))
    declared = native.declared_symbols()
    for name in ("kp1_dock_curriculum_create_population", "kp1_dock_curriculum_observe_population", "kp1_dock_curriculum_read_replica"):
        assert hasattr(lib, name), name
        assert name in declared, name


def _header_fields(struct: str) -> list[str]:
    """member names of `typedef struct <struct> {...}` in include/kp1_ppo.h, in order"""
    text = (native.PKG_DIR.parent / "include" / "kp1_ppo.h").read_text()
    body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        decl = re.sub(r"^\s*\w+\s+", "", decl)          # drop the type
        names += [re.sub(r"\[.*?\]", "", n).strip() for n in decl.split(",")]
    return names


def test_dock_tracker_ctypes_layouts_match_the_header():
    """finisher_tools' _Stage / _Event / _State mirror kp1_dock_curriculum_stage / _event / _state member for member, and the population
    allocation (K trackers, then K live stage records) puts record k at K * sizeof(state) + k * sizeof(stage) with the records 8-byte aligned"""
    from rl_brain_trainer_amd import finisher_tools as ft

    for cls, struct in ((ft._Stage, "kp1_dock_curriculum_stage"), (ft._Event, "kp1_dock_curriculum_event"), (ft._State, "kp1_dock_curriculum_state")):
        assert [f[0] for f in cls._fields_] == _header_fields(struct), struct
    assert C.sizeof(ft._Stage) == 23 * 8 + 4 * 4
    assert C.sizeof(ft._State) % C.alignment(ft._Stage) == 0
    assert ft._Stage.handoff_count.offset == C.sizeof(ft._Stage) - 4


def test_dock_population_classes():
    from rl_brain_trainer_amd.finisher_tools import DockReverseCurriculum, DockReverseCurriculumPopulation
    from rl_brain_trainer_amd.population import DockPopulationPPO, OneHandlePopulationPPO, RoutePopulationPPO

    assert issubclass(DockPopulationPPO, OneHandlePopulationPPO)
    assert issubclass(DockReverseCurriculumPopulation, DockReverseCurriculum)
    for name in ("check_init_checkpoint", "check_init_checkpoints", "load_init_checkpoint", "load_init_checkpoints"):
        assert name in OneHandlePopulationPPO.__dict__, name
        assert name not in RoutePopulationPPO.__dict__ and name not in DockPopulationPPO.__dict__, name


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to create a device handle fails the test: the refusals below must come first"""
    import torch

    def touched(*_a, **_k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(torch.cuda, "is_available", touched)
    monkeypatch.setattr(native, "load", touched)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)


def test_dock_population_refusals_before_device_work(no_device):
    from rl_brain_trainer_amd import config as kcfg
    from rl_brain_trainer_amd.finisher_tools import DockReverseCurriculumPopulation
    from rl_brain_trainer_amd.population import DockPopulationPPO
    from rl_brain_trainer_amd.ppo import PPOConfig
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    with pytest.raises(ValueError, match="1 to 16"):
        DockReverseCurriculumPopulation(stages=[{"name": "a"}], window_episodes=4, n_replicas=17)
    with pytest.raises(TypeError, match="dock-mode ArmKinematicPopulationVecEnv"):
        DockPopulationPPO([7, 8], PPOConfig(hidden=64), object())
    with pytest.raises(ValueError, match="teacher-anchor"):
        DockPopulationPPO([7, 8], PPOConfig(hidden=64), object(), teacher_anchor=object())
    approach = kcfg.to_env_config(kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"))
    with pytest.raises(ValueError, match="approach-mode config"):
        ArmKinematicPopulationVecEnv(approach, [7, 8], 12, mode="dock")
    dock = kcfg.to_env_config(kcfg.load_yaml_file(kcfg.builtin_config_dir() / "dock_workspace_handoff_noop_ft_12env.yaml"))
    with pytest.raises(ValueError, match="f32"):
        ArmKinematicPopulationVecEnv(dock, [7, 8], 12, mode="dock", real="f64")


# ---------------------------------------------------------------------------------------------------------------- --resume-from
def _write_checkpoint(path, *, hidden: int = 64, adam_steps: int = 10, num_timesteps: int = 3072, actor_extra_steps: int = 0) -> None:
    """a checkpoint zip of a 2 x hidden dock policy: policy.pth, an Adam state of `adam_steps` steps (the actor tensors `actor_extra_steps`
    more) and SB3's data member with num_timesteps"""
    import torch

    from rl_brain_trainer_amd.ppo import ActorCritic

    pol = ActorCritic(hidden, torch.device("cpu"))
    state = {}
    for i, (name, shape) in enumerate(pol.spec):
        actor = name.startswith(("mlp_extractor.policy_net", "action_net"))
        state[i] = {"step": torch.tensor(float(adam_steps + (actor_extra_steps if actor else 0))), "exp_avg": torch.zeros(shape),
                    "exp_avg_sq": torch.zeros(shape)}
    opt = {"state": state, "param_groups": [{"params": list(range(len(pol.spec)))}]}
    buf_p, buf_o = io.BytesIO(), io.BytesIO()
    torch.save(pol.state_dict(), buf_p)
    torch.save(opt, buf_o)
    path.parent.mkdir(parents=True, exist_ok=True)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", buf_p.getvalue())
        z.writestr("policy.optimizer.pth", buf_o.getvalue())
        z.writestr("data", json.dumps({"num_timesteps": num_timesteps, "n_epochs": 5, "_n_updates": 20}))


def _root(tmp_path, seeds, **per_seed) -> str:
    """an earlier --seeds run root: seed_<s>/model_latest.zip per seed (per_seed[s]: _write_checkpoint overrides of seed s)"""
    root = tmp_path / "phase1"
    for s in seeds:
        _write_checkpoint(root / f"seed_{s}" / "model_latest.zip", **per_seed.get(f"s{s}", {}))
    return str(root)


def test_resume_from_resolution(tmp_path, no_device):
    from rl_brain_trainer_amd.population import resolve_resume_population

    root = _root(tmp_path, [3, 4, 5])
    assert resolve_resume_population(root, [3, 4, 5]) == [f"{root}/seed_{s}/model_latest.zip" for s in (3, 4, 5)]
    assert resolve_resume_population(root, [5, 3]) == [f"{root}/seed_{s}/model_latest.zip" for s in (5, 3)]
    one = tmp_path / "one.zip"
    _write_checkpoint(one)
    assert resolve_resume_population(str(one), [3, 4]) == [str(one), str(one)]
    # as a --seed run does, a path that does not exist starts from scratch
    assert resolve_resume_population(str(tmp_path / "nowhere"), [3, 4]) is None
    assert resolve_resume_population(None, [3, 4]) is None


@pytest.mark.parametrize("per_seed, seeds, match", [
    ({}, [3, 4, 6], r"seeds \[6\]"),
    ({"s4": {"adam_steps": 11}}, [3, 4], "Adam step counts"),
    ({"s4": {"num_timesteps": 6144}}, [3, 4], "num_timesteps"),
    ({"s3": {"hidden": 256}, "s4": {"hidden": 256}}, [3, 4], "2x256"),
    ({"s3": {"hidden": 128}}, [3, 4], "hidden widths"),
    ({"s3": {"actor_extra_steps": 4}}, [3, 4], "actor_extra_steps"),
])
def test_resume_from_directory_refusals(tmp_path, no_device, per_seed, seeds, match):
    from rl_brain_trainer_amd.population import resolve_resume_population

    root = _root(tmp_path, [3, 4, 5], **per_seed)
    with pytest.raises(ValueError, match=match):
        resolve_resume_population(root, seeds)


def test_train_dock_seeds_resume_refusals_come_first(tmp_path, no_device):
    """train_dock --seeds --resume-from refuses a root missing a seed and a teacher-anchored zip before it touches a device"""
    import yaml

    from rl_brain_trainer_amd import config as kcfg, train_dock

    dock = kcfg.load_yaml_file(kcfg.builtin_config_dir() / "dock_workspace_handoff_noop_ft_12env.yaml")
    cfg_path = tmp_path / "dock.yaml"
    cfg_path.write_text(yaml.safe_dump(dock))
    common = ["--config", str(cfg_path), "--n-envs", "12", "--hidden", "64", "--artifact-root", str(tmp_path / "out")]
    root = _root(tmp_path, [3, 4])
    with pytest.raises(ValueError, match=r"seeds \[5\]"):
        train_dock.main(common + ["--seeds", "3,4,5", "--resume-from", root])
    anchored = tmp_path / "anchored.zip"
    _write_checkpoint(anchored, actor_extra_steps=2)
    with pytest.raises(ValueError, match="actor_extra_steps"):
        train_dock.main(common + ["--seeds", "3,4", "--resume-from", str(anchored)])
    wide = tmp_path / "wide.zip"
    _write_checkpoint(wide, hidden=256)
    with pytest.raises(ValueError, match="2x256"):
        train_dock.main(common + ["--seeds", "3,4", "--resume-from", str(wide)])
