"""Route-stride Approach resets (env.route_reset), CPU part: the numpy restatement (tests/route_stride_reset.py) against the reference's own
record (tests/golden/route_stride_resets.npz, made by make_golden_route_stride_reset.py) bit for bit, the census of the forced classes, the
config parser and the route loader with their refusals, and the C ABI symbol.  The GPU part (test_route_stride_reset_gpu.py) runs the
kernels against the fixture rows and, on ordinary seeds, against the restatement; it imports the fixture plumbing from here."""
from __future__ import annotations

import copy
import ctypes as C
import json
from functools import lru_cache

import numpy as np
import pytest

import rng_forcing as rf
import route_stride_reset as rsr
from conftest import GOLDEN
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import native

SCENE = "approach_scene_route_curriculum_tray1_h1_to_h8_12env"
# every class the fixture must hold, each at least twice (DESIGN section 36's census)
CLASSES = ("stream", "half_per_reset", "nodraw", "always_reversed", "clipped", "rot0", "rot63", "stride_lemire_zero", "stride_lemire_reject",
           "stride_lemire_at_threshold", "start_lemire_zero", "start_lemire_reject", "start_lemire_at_threshold", "u_zero", "u_boundary_minus",
           "u_boundary", "u_boundary_plus", "u_max")


# ============================================================================== fixture plumbing (shared with the GPU tests)
@lru_cache(maxsize=None)
def fixture() -> dict:
    g = np.load(GOLDEN / "route_stride_resets.npz")
    out = {k: g[k] for k in g.files if k != "groups"}
    meta = json.loads(str(g["groups"]))
    assert meta["config"] == SCENE
    out["groups"] = meta["groups"]
    return out


def rows_of(group: str, stage: int | None = None) -> np.ndarray:
    f = fixture()
    return np.flatnonzero((f["group"] == group) & ((f["stage"] == stage) if stage is not None else True))


def scene_dict() -> dict:
    return json.loads((GOLDEN / "configs" / f"{SCENE}.json").read_text())


def group_cfg_dict(group: str, extra: dict | None = None) -> dict:
    """the scene config with the group's overrides ("a.b.c": value) applied, then `extra`"""
    cfg = copy.deepcopy(scene_dict())
    for path, value in {**fixture()["groups"][group]["overrides"], **(extra or {})}.items():
        node = cfg
        keys = path.split(".")
        for k in keys[:-1]:
            node = node.setdefault(k, {})
        node[keys[-1]] = value
    return cfg


@lru_cache(maxsize=None)
def group_env_config(group: str) -> kcfg.EnvConfig:
    return kcfg.to_env_config(group_cfg_dict(group), handoff_base_dirs=(GOLDEN,))


def restate(group: str, stage: int, w) -> dict:
    """the numpy restatement of one reset of the group from the words `w`"""
    ec = group_env_config(group)
    bg = rf.bitgen_of(w)
    lower, upper = np.array(ec.c.joints.lower[:]), np.array(ec.c.joints.upper[:])
    q, gq, start, goal = rsr.sample(np.random.Generator(bg), np.array(ec.route_reset.route_q), group_cfg_dict(group)["env"]["route_reset"], stage, lower, upper)
    return {"initial_q": q, "goal_q": gq, "indices": np.array([start, goal]), "words_after": rf.words_of(bg)}


# ============================================================================== the restatement and the census
def test_restatement_equals_every_fixture_row():
    f = fixture()
    assert len(f["group"]) >= 250
    for j in range(len(f["group"])):
        got = restate(str(f["group"][j]), int(f["stage"][j]), f["words_before"][j])
        for k in ("initial_q", "goal_q", "indices", "words_after"):
            assert np.array_equal(got[k], f[k][j]), (str(f["label"][j]), k)


def test_fixture_census_and_branches():
    f = fixture()
    for cls in CLASSES:
        rows = np.flatnonzero(f["cls"] == cls)
        assert rows.size >= 2, cls
        for j in rows:
            w, label = f["words_before"][j], str(f["label"][j])
            got = rf.classify(w, json.loads(str(f["draws"][j])))
            for at, want in json.loads(str(f["expect"][j])):
                assert got[at][0] == want, (label, at, want, got[at])
            if f["u_k"][j] >= 0:
                assert rf.generator_of(w).random() == int(f["u_k"][j]) * 2.0 ** -53, label
            if cls in ("rot0", "rot63"):
                bg = rf.bitgen_of(w)
                bg.random_raw()
                assert int(rf.words_of(bg)[0]) >> 58 == (0 if cls == "rot0" else 63), label
    assert set(f["cls"]) == set(CLASSES)
    # the branches the groups exist for
    start, goal = f["indices"][:, 0], f["indices"][:, 1]
    for j in np.flatnonzero(f["cls"] == "nodraw"):
        assert np.array_equal(f["words_before"][j], f["words_after"][j]) and f["halves"][j] == 0 and (start[j], goal[j]) == (0, 2)
    assert set(f["stage"][f["cls"] == "nodraw"]) == {1, 2}
    hp = np.flatnonzero(f["cls"] == "half_per_reset")
    assert np.all(f["halves"][hp] == 1)
    assert [rf.lcg_steps(f["words_before"][j], f["words_after"][j]) for j in hp] == [1, 0] * (hp.size // 2)    # the carried 32-bit half
    rev = np.flatnonzero(f["cls"] == "always_reversed")
    assert np.all(start[rev] == goal[rev] + 1) and np.all(f["halves"][rev] == 17)
    lo, hi = np.array(group_env_config("scene").c.joints.lower[:]), np.array(group_env_config("scene").c.joints.upper[:])
    for j in np.flatnonzero(f["cls"] == "clipped"):
        assert np.sum((f["initial_q"][j] == lo) | (f["initial_q"][j] == hi)) >= 2
    for cls, swapped in (("u_zero", True), ("u_boundary_minus", True), ("u_boundary", False), ("u_boundary_plus", False), ("u_max", False)):
        rows = np.flatnonzero(f["cls"] == cls)
        assert np.all((start[rows] > goal[rows]) == swapped), cls             # strict "<": the row ON the boundary is not reversed
    k = rf.k_of(0.125)
    assert sorted(set(f["u_k"][f["u_k"] >= 0])) == [0, k - 1, k, k + 1, rf.ONE_BELOW]
    for stage, (a, b) in {0: (1, 1), 3: (8, 10), 5: (16, 28)}.items():
        rows = rows_of("scene", stage)
        rows = rows[f["cls"][rows] == "stream"]
        assert rows.size == 64 and np.all((np.abs(goal[rows] - start[rows]) >= a) & (np.abs(goal[rows] - start[rows]) <= b))
        assert np.array_equal(f["words_before"][rows[1:]], f["words_after"][rows[:-1]])      # consecutive resets of one env


# ============================================================================== config parser and route loader
def test_scene_config_is_accepted():
    ec = kcfg.to_env_config(scene_dict(), handoff_base_dirs=(GOLDEN,))
    rr = ec.route_reset
    assert rr.active and rr.enabled and len(rr.route_q) == 484 and rr.route_path == "synthetic_route.json"
    assert rr.min_stride_by_stage == (1, 2, 4, 8, 12, 16) and rr.max_stride_by_stage == (1, 3, 6, 10, 18, 28)
    assert rr.start_q_noise == rr.goal_q_noise == (0.002,) + (0.006,) * 6 and rr.reverse_probability == 0.10
    assert ec.mode_name == "approach" and ec.n_stages == 6 and ec.c.curriculum_enabled == 1
    assert ec.clone().route_reset is rr


def test_defaults_and_disabled_block_change_nothing():
    rr = kcfg.RouteResetConfig()
    assert (rr.enabled, rr.route_path, rr.min_stride_by_stage, rr.max_stride_by_stage, rr.reverse_probability, rr.route_q) == (False, "", (1,), (1,), 0.0, ())
    assert rr.start_q_noise == rr.goal_q_noise == (0.0,) * 7 and not rr.active
    base = scene_dict()
    absent = copy.deepcopy(base)
    del absent["env"]["route_reset"]
    off = copy.deepcopy(base)
    off["env"]["route_reset"]["enabled"] = False
    off["env"]["route_reset"]["route_path"] = "no/such/file.json"       # a disabled block does not load its route
    a, b = kcfg.to_env_config(absent), kcfg.to_env_config(off)
    assert bytes(a.c) == bytes(b.c) and not a.route_reset.active and not b.route_reset.active and b.route_reset.route_q == ()
    assert a.route_reset == kcfg.RouteResetConfig()
    on = kcfg.to_env_config(base, handoff_base_dirs=(GOLDEN,))
    assert bytes(on.c) == bytes(a.c)                                     # the block lives beside the C struct, which keeps its layout and values
    with pytest.raises(TypeError, match="unexpected keyword argument 'stride'"):
        kcfg.to_env_config(group_cfg_dict("scene", {"env.route_reset.stride": 3}), handoff_base_dirs=(GOLDEN,))


@pytest.mark.parametrize("shape", ["route_q", "waypoints", "bare", "q_items"])
def test_route_file_shapes(shape, tmp_path, monkeypatch):
    pts = [[0.01 * i + 0.001 * k for k in range(7)] for i in range(5)]
    payload = {"route_q": {"route_q": pts}, "waypoints": {"waypoints": pts}, "bare": pts, "q_items": {"waypoints": [{"q": p, "name": "w"} for p in pts]}}[shape]
    (tmp_path / "r.json").write_text(json.dumps(payload))
    want = tuple(tuple(p) for p in pts)
    assert kcfg.load_route_q(str(tmp_path / "r.json")) == want                           # absolute
    assert kcfg.load_route_q("r.json", base_dirs=(tmp_path / "nowhere", tmp_path)) == want   # a base dir
    monkeypatch.chdir(tmp_path)
    assert kcfg.load_route_q("r.json") == want                                           # the working directory
    cfg = group_cfg_dict("scene", {"env.route_reset.route_path": str(tmp_path / "r.json"), "env.route_reset.min_stride_by_stage": [1, 2],
                                   "env.route_reset.max_stride_by_stage": [4]})
    assert kcfg.to_env_config(cfg).route_reset.route_q == want


def test_loader_errors(tmp_path):
    assert kcfg.load_route_q("") == ()
    with pytest.raises(FileNotFoundError, match="Route reset path does not exist"):
        kcfg.load_route_q(str(tmp_path / "missing.json"))
    with pytest.raises(FileNotFoundError, match="Route reset path does not exist"):
        kcfg.to_env_config(group_cfg_dict("scene", {"env.route_reset.route_path": "missing.json"}), handoff_base_dirs=(tmp_path,))
    (tmp_path / "one.json").write_text(json.dumps({"route_q": [[0.0] * 7]}))
    with pytest.raises(ValueError, match="at least two q waypoints"):
        kcfg.load_route_q(str(tmp_path / "one.json"))
    (tmp_path / "six.json").write_text(json.dumps({"route_q": [[0.0] * 6, [0.0] * 6]}))
    with pytest.raises(ValueError, match="7-joint vectors"):
        kcfg.load_route_q(str(tmp_path / "six.json"))
    with pytest.raises(ValueError, match="7-joint vectors"):
        kcfg.to_env_config(group_cfg_dict("scene", {"env.route_reset.start_q_noise": [0.0] * 6}), handoff_base_dirs=(GOLDEN,))


def test_infeasible_stride_is_refused_naming_the_stage():
    """three points, the scene's strides: stage 2 asks for a stride of 4 and the route allows 2 -- the reference raises `low >= high` at that
    stage's first reset, the parser when the config is read"""
    with pytest.raises(ValueError, match=r"stage 2 needs a stride of at least 4.*3 points allows 2"):
        kcfg.to_env_config(group_cfg_dict("scene", {"env.route_reset.route_path": "route_three_points.json"}), handoff_base_dirs=(GOLDEN,))
    # the last entry serves every later stage: [1, 3] on three points fails from stage 1 on
    with pytest.raises(ValueError, match=r"stage 1 needs a stride of at least 3"):
        kcfg.to_env_config(group_cfg_dict("tiny_nodraw", {"env.route_reset.min_stride_by_stage": [1, 3]}), handoff_base_dirs=(GOLDEN,))
    with pytest.raises(ValueError, match="holds 1..16 entries"):
        kcfg.to_env_config(group_cfg_dict("tiny_nodraw", {"env.route_reset.max_stride_by_stage": [1] * 17}), handoff_base_dirs=(GOLDEN,))
    with pytest.raises(ValueError, match="must not be negative"):
        kcfg.to_env_config(group_cfg_dict("tiny_nodraw", {"env.route_reset.goal_q_noise": [0.0] * 6 + [-0.1]}), handoff_base_dirs=(GOLDEN,))
    assert kcfg.to_env_config(group_cfg_dict("tiny_nodraw"), handoff_base_dirs=(GOLDEN,)).route_reset.active      # max 9 is clamped to P - 1, not refused


# ============================================================================== the C ABI symbol
def test_symbol_is_declared_exported_and_bound():
    name = "kp1_set_route_stride_reset"
    assert name in native.declared_symbols()
    fn = getattr(native.load(), name)
    assert fn.restype is C.c_int32
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double]
    assert native.load().kp1_abi_version() == 1
    assert fn(None, None, 0, None, 0, None, 0, None, None, 0.0) == -1                      # a NULL handle is refused before any device call
    assert b"env is NULL" in native.load().kp1_last_error()
