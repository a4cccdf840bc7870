"""The population teacher-anchor step without a GPU: the two entry points are exported, declared and bound with matching argument lists and
refuse NULL arguments before any device call; PopulationTeacherAnchor draws RouteTeacherAnchor's index stream and validates its dataset on
the host; the populations' refusals."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import abi
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import route_config as rcfg
from rl_brain_trainer_amd.ppo import PPOConfig
from rl_brain_trainer_amd.teacher_anchor import PopulationTeacherAnchor, RouteTeacherAnchor, TeacherAnchorConfig

ANCHOR_SYMBOLS = {"kp1_mlp_anchor_loss_grad": 10, "kp1_mlp_anchor_adam_step": 10}


def test_anchor_symbols_exported_declared_and_bound():
    lib = C.CDLL(str(native.LIB_PATH))
    L = native.load()
    for name, n_args in ANCHOR_SYMBOLS.items():
        assert hasattr(lib, name), name
        assert name in native.declared_symbols(), name
        params = abi.params(name, "kp1_ppo.h")
        assert len(getattr(L, name).argtypes) == len(params) == n_args, name
        for text, ctype in zip(params, getattr(L, name).argtypes):
            if "*" in text:
                assert ctype is C.c_void_p, text
            elif "float" in text:
                assert ctype is C.c_float, text
            else:
                assert "int32_t" in text and ctype is C.c_int32, text


def test_anchor_library_refuses_null_arguments_before_any_device_call():
    L = native.load()
    dummy = (C.c_int32 * 4)(1, 1, 1, 1)
    p = C.cast(dummy, C.c_void_p)
    assert L.kp1_mlp_anchor_loss_grad(None, p, 128, None, 4, p, 0.5, p, p, None) != native.KP1_OK and b"NULL" in L.kp1_last_error()
    assert L.kp1_mlp_anchor_adam_step(None, p, p, p, p, 3e-4, 1e-5, 0.5, 1, None) != native.KP1_OK and b"NULL" in L.kp1_last_error()


def _write_dataset(path, rows: int, seed: int = 0) -> None:
    g = np.random.default_rng(seed)
    obs = g.uniform(-1, 1, (rows, rcfg.ROUTE_OBS_DIM)).astype(np.float32)
    np.savez(path, actions=g.uniform(-1, 1, (rows, 7)).astype(np.float32), route_index=(np.arange(rows) % 30).astype(np.int32),
             **{f"obs__{k}": obs[:, o:o + w] for k, (o, w) in rcfg.ROUTE_OBS_LAYOUT.items()})


@pytest.mark.parametrize("rows, batch", [(600, 256), (90, 256)])
def test_population_anchor_draws_the_single_anchor_index_stream(tmp_path, rows, batch):
    """three calls of sample_indices: the same default_rng(0) stream over the same M, full batches and M < batch_size"""
    import torch

    path = tmp_path / "teacher.npz"
    _write_dataset(path, rows)
    cfg = TeacherAnchorConfig(enabled=True, dataset_path=str(path), batch_size=batch, max_route_index=19)
    pop_anchor = PopulationTeacherAnchor(cfg)
    single = RouteTeacherAnchor(cfg)
    kept = rows * 20 // 30
    single._actions = torch.zeros((kept, 7))        # what on_training_start leaves: the filtered dataset's actions
    assert pop_anchor.rows == kept and pop_anchor.batch_rows == min(batch, kept)
    assert pop_anchor.summary()["sample_count"] == kept and pop_anchor.summary()["enabled"] is True
    for _ in range(3):
        a, b = pop_anchor.sample_indices(), single.sample_indices()
        assert a.shape == (min(batch, kept),) and np.array_equal(a, b)


def test_population_anchor_validates_the_dataset_on_the_host(tmp_path, monkeypatch):
    import torch

    def touched(*_a, **_k):
        raise AssertionError("torch.cuda was touched before the dataset was validated")

    for name in ("set_device", "current_stream", "synchronize", "is_available", "device_count"):
        monkeypatch.setattr(torch.cuda, name, touched)
    with pytest.raises(ValueError, match="teacher-anchor"):
        PopulationTeacherAnchor(TeacherAnchorConfig(enabled=True, dataset_path=str(tmp_path / "none.npz")))
    with pytest.raises(ValueError, match="teacher-anchor"):
        PopulationTeacherAnchor(TeacherAnchorConfig(enabled=True, dataset_path=""))
    (tmp_path / "garbage.npz").write_bytes(b"not a zip archive")
    with pytest.raises(ValueError, match="teacher-anchor"):
        PopulationTeacherAnchor(TeacherAnchorConfig(enabled=True, dataset_path=str(tmp_path / "garbage.npz")))
    np.savez(tmp_path / "keys.npz", actions=np.zeros((3, 7), np.float32))
    with pytest.raises(ValueError, match="teacher-anchor"):
        PopulationTeacherAnchor(TeacherAnchorConfig(enabled=True, dataset_path=str(tmp_path / "keys.npz")))
    _write_dataset(tmp_path / "late.npz", 40)
    with pytest.raises(ValueError, match="teacher-anchor dataset .* no samples left"):
        PopulationTeacherAnchor(TeacherAnchorConfig(enabled=True, dataset_path=str(tmp_path / "late.npz"), max_route_index=-1))


def test_populations_refuse_what_is_not_a_population_anchor(tmp_path):
    from rl_brain_trainer_amd.population import ApproachPopulationPPO, DockPopulationPPO, PopulationPPO, RoutePopulationPPO

    _write_dataset(tmp_path / "teacher.npz", 64)
    cfg = TeacherAnchorConfig(enabled=True, dataset_path=str(tmp_path / "teacher.npz"), max_route_index=19)
    real = PopulationTeacherAnchor(cfg)
    for other in (object(), RouteTeacherAnchor(cfg)):
        with pytest.raises(ValueError, match="teacher-anchor"):
            RoutePopulationPPO([7, 8], PPOConfig(hidden=64), None, teacher_anchor=other)
    # a real anchor passes the shared refusals of a route population: the next refusal is the env type
    with pytest.raises(TypeError, match="RoutePopulationVecEnv"):
        RoutePopulationPPO([7, 8], PPOConfig(hidden=64), None, teacher_anchor=real)
    # the anchor is a route feature: the other populations refuse it, real or not
    for anchor in (object(), real):
        with pytest.raises(ValueError, match="teacher-anchor"):
            ApproachPopulationPPO([7, 8], PPOConfig(hidden=64), None, teacher_anchor=anchor)
        with pytest.raises(ValueError, match="teacher-anchor"):
            DockPopulationPPO([7, 8], PPOConfig(hidden=64), None, teacher_anchor=anchor)
        with pytest.raises(ValueError, match="teacher-anchor"):
            PopulationPPO([7, 8], PPOConfig(hidden=64), lambda s: None, teacher_anchor=anchor)
