"""Population PPO without a GPU: the population ABI is exported, and PopulationPPO refuses what it does not support before touching a device."""
from __future__ import annotations

import ctypes as C

import pytest

from rl_brain_trainer_amd import native
from rl_brain_trainer_amd.ppo import PPOConfig


def test_population_symbols_exported():
    lib = C.CDLL(str(native.LIB_PATH))
    for name in ("kp1_mlp_create_population", "kp1_mlp_replicas"):
        assert hasattr(lib, name), name
        assert name in native.declared_symbols(), name
    lib.kp1_mlp_replicas.argtypes = [C.c_void_p]
    lib.kp1_mlp_replicas.restype = C.c_int32
    assert lib.kp1_mlp_replicas(None) == 0
    header = (native.PKG_DIR.parent / "include" / "kp1_ppo.h").read_text()
    assert "#define KP1_MLP_MAX_REPLICAS 16" in header


class _FakeEnv:
    """what PopulationPPO reads from an env before it refuses one"""

    def __init__(self, obs_dim=56):
        import torch

        self.obs_dim, self.dtype, self.n_envs, self.closed = obs_dim, torch.float32, 4, False

    def close(self):
        self.closed = True


class _EnabledDist:
    enabled, world_size, rank = True, 2, 0


def _unused_factory(seed):
    raise AssertionError("the env factory must not be called for a refused configuration")


@pytest.mark.parametrize("seeds, cfg, kwargs, match", [
    ([7, 8], PPOConfig(hidden=256), {}, "hidden=256"),
    ([7, 7], PPOConfig(), {}, "distinct"),
    (list(range(17)), PPOConfig(), {}, "at most 16"),
    ([], PPOConfig(), {}, "at least one"),
    ([7, 8], PPOConfig(), {"teacher_anchor": object()}, "teacher-anchor"),
    ([7, 8], PPOConfig(), {"dist": _EnabledDist()}, "data parallel"),
])
def test_population_refusals(seeds, cfg, kwargs, match):
    from rl_brain_trainer_amd.population import PopulationPPO

    with pytest.raises(ValueError, match=match):
        PopulationPPO(seeds, cfg, _unused_factory, **kwargs)


def test_population_refuses_route_envs():
    from rl_brain_trainer_amd.population import PopulationPPO

    made = []

    def factory(seed):
        made.append(_FakeEnv(obs_dim=80))
        return made[-1]

    with pytest.raises(ValueError, match="route envs"):
        PopulationPPO([7, 8], PPOConfig(), factory)
    assert made and all(e.closed for e in made)


@pytest.mark.parametrize("module", ["train", "train_dock"])
def test_seeds_and_seed_exclude_each_other(module, capsys):
    import importlib

    mod = importlib.import_module(f"rl_brain_trainer_amd.{module}")
    parser = mod.build_arg_parser()
    args = parser.parse_args(["--config", "c.yaml", "--seeds", "7,8,9,10"])
    assert args.seeds == "7,8,9,10" and args.seed is None
    assert parser.parse_args(["--config", "c.yaml", "--seed", "7"]).seeds is None
    with pytest.raises(SystemExit):
        parser.parse_args(["--config", "c.yaml", "--seed", "7", "--seeds", "7,8"])
    assert "not allowed with argument" in capsys.readouterr().err


def test_parse_seeds():
    from rl_brain_trainer_amd.population import parse_seeds

    assert parse_seeds("7,8, 9,10") == [7, 8, 9, 10]
    with pytest.raises(ValueError):
        parse_seeds("7,x")
    with pytest.raises(ValueError):
        parse_seeds(",")
