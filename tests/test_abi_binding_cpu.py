"""The Python <-> C boundary is derived from include/kp1.h, kp1_ppo.h and kp1_route.h, checked without a GPU: every
prototype is exported and bound with its parameter count and types, the prototype parser and ``header_int`` on synthetic text, the mirrored
constants at the values they had as literals, and every ctypes mirror of a header struct against ``offsetof`` / ``sizeof`` as the host C
compiler lays the struct out."""
from __future__ import annotations

import ctypes as C
import importlib
import inspect
import os
import shutil
import subprocess

import pytest

import abi
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import curriculum, finisher_tools, mlp, native, population, ppo, rccl, route_config, route_curriculum, route_env, vec_env

PROTOS = abi.prototypes()
SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
RETURNS = {**SCALARS, "void": None, "const char *": C.c_char_p}


def test_the_headers_declare_at_least_the_parents_functions():
    assert len(PROTOS) >= 126
    assert sorted(PROTOS) == sorted(native.declared_symbols())
    assert len(native.declared_symbols()) == len(set(native.declared_symbols()))


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_every_prototype_is_exported_and_bound(name):
    ret, params = PROTOS[name]
    assert hasattr(C.CDLL(str(native.LIB_PATH)), name), f"libkp1.so does not export {name}"
    fn = getattr(native.load(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, params)
    assert fn.restype is RETURNS[ret], (name, ret)
    for text, ctype in zip(params, fn.argtypes):
        words = [w for w in text.replace("*", " * ").split() if w != "const"]
        if words.count("*") == 0:
            assert ctype is SCALARS[words[0]], (name, text)
        elif words.count("*") == 2:
            assert ctype is C.POINTER(C.c_void_p), (name, text)
        else:
            assert ctype is C.c_void_p or (issubclass(ctype, C._Pointer) and ctype._type_ in (C.c_int32, *native.struct_registry().values())), (name, text)


def test_registered_struct_pointers_are_typed():
    L = native.load()
    assert L.kp1_create.argtypes[0] is C.POINTER(kcfg.Kp1Config) and L.kp1_reset.argtypes[2] is C.POINTER(kcfg.ResetOpts)
    assert L.kp1_get_info.argtypes[1] is C.POINTER(kcfg.InfoView) and L.kp1_get_stage.argtypes[1] is C.POINTER(C.c_int32)
    assert L.kp1_route_create.argtypes[1] is C.POINTER(route_config.RouteConfig)
    assert L.kp1_route_reset.argtypes[2] is C.POINTER(route_env._RouteResetOpts) and L.kp1_route_get_info.argtypes[1] is C.POINTER(route_env._RouteInfoView)
    assert L.kp1_dock_curriculum_create.argtypes[1] is C.POINTER(finisher_tools._Stage)
    # the tracker handles are device memory of the struct's type (the headers' *_dev parameters): void*; the host copy is the mirror
    assert list(L.kp1_dock_curriculum_read.argtypes) == [C.c_void_p, C.c_void_p, C.POINTER(finisher_tools._State), C.c_void_p]
    assert list(L.kp1_route_curriculum_read_replica.argtypes) == [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(route_curriculum._CurriculumState), C.c_void_p]
    # one type for kp1_rng_state in all five functions that take it
    for name in ("kp1_rng_get", "kp1_rng_set", "kp1_route_rng_get", "kp1_route_rng_set", "kp1_rng_seed_state"):
        assert getattr(L, name).argtypes[1] is C.POINTER(kcfg.RngState), name
    assert L.kp1_mlp_num_params_ex.restype is C.c_int64 and L.kp1_mlp_num_params.restype is C.c_int64
    assert list(L.kp1_mlp_loss_grad.argtypes[9:11]) == [C.c_float, C.c_float] and L.kp1_mlp_loss_grad.argtypes[18] is C.c_int32


# ------------------------------------------------------------------------------------------------ the parser on synthetic text
class _Mirror(C.Structure):
    _fields_ = [("a", C.c_int32)]


SYNTHETIC = """
typedef struct kp1_thing kp1_thing;          // an opaque handle (not a function, whatever follows: kp1_no(int x);)
typedef struct kp1_mirror { int32_t a; } kp1_mirror;
/* kp1_commented_out(int a, float b); takes (a, b) */
int kp1_spread(kp1_thing* h,        /* the handle (opaque, as in f(x, y)) */
               const float* in,     // read, (n) floats
               float const* also_in,
               int32_t n, void* stream);
const char* kp1_name(void);
uint64_t kp1_size();
int kp1_out(kp1_thing** out, const void** views, int32_t* count);
int kp1_get_stage(const kp1_thing*, int32_t*);
void kp1_fill(kp1_mirror* m, const struct kp1_mirror* src, kp1_mirror* table_dev, int64_t, double, uint64_t big, float);
"""


def test_parser_on_synthetic_text():
    vp = C.c_void_p
    got = native.parse_prototypes(SYNTHETIC, {"kp1_mirror": _Mirror})
    assert got == {"kp1_spread": (C.c_int32, [vp, vp, vp, C.c_int32, vp]),
                   "kp1_name": (C.c_char_p, []), "kp1_size": (C.c_uint64, []),
                   "kp1_out": (C.c_int32, [C.POINTER(vp), C.POINTER(vp), vp]),
                   "kp1_get_stage": (C.c_int32, [vp, C.POINTER(C.c_int32)]),
                   "kp1_fill": (None, [C.POINTER(_Mirror), C.POINTER(_Mirror), vp, C.c_int64, C.c_double, C.c_uint64, C.c_float])}


@pytest.mark.parametrize("proto, part", [("int kp1_bad(unsigned n);", "unsigned n"), ("int kp1_bad(kp1_thing h);", "kp1_thing h"),
                                         ("int kp1_bad(long long n);", "long long n"), ("int kp1_bad(float v[4]);", "float v[4]"),
                                         ("int kp1_bad(int32_t*** p);", "int32_t*** p"), ("size_t kp1_bad(void);", "size_t"),
                                         ("float* kp1_bad(void);", "float*")])
def test_parser_refuses_what_it_does_not_know(proto, part):
    with pytest.raises(native.Kp1Error) as e:
        native.parse_prototypes(proto, {})
    assert "kp1_bad" in str(e.value) and part in str(e.value)


def test_missing_header_is_an_error(monkeypatch, tmp_path):
    (tmp_path / "include").mkdir()
    shutil.copy(kcfg.repo_root() / "include" / "kp1.h", tmp_path / "include" / "kp1.h")
    monkeypatch.setattr(kcfg, "repo_root", lambda: tmp_path)
    native.header_text.cache_clear()
    try:
        with pytest.raises(native.Kp1Error) as e:
            native.header_text()
        assert str(tmp_path / "include" / "kp1_ppo.h") in str(e.value)
    finally:
        native.header_text.cache_clear()


# ------------------------------------------------------------------------------------------------ constants
def test_header_int_forms_and_refusals():
    text = "#define A 914  /* (1 << 3) */\n#  define B 0x1F // 7\n#define C_ (1 << 10)\n#define D (2 * 8)\n#define E 1.5\n#define F\n#define G A\n#define AA 3\n"
    assert [native.header_int(n, text) for n in ("A", "B", "C_", "AA")] == [914, 31, 1024, 3]
    for name in ("D", "E", "F", "G", "MISSING"):
        with pytest.raises(native.Kp1Error) as e:
            native.header_int(name, text)
        assert name in str(e.value)
    assert native.header_int("KP1_MONITOR_MAX_STEPS") == 4096
    with pytest.raises(native.Kp1Error):
        native.header_int("KP1_NO_SUCH_DEFINE")
    with pytest.raises(native.Kp1Error):
        native.header_int("KP1_UNSET")      # (-2147483647 - 1): an expression


def test_mirrored_constants_keep_their_values():
    assert (native.EVAL_EPISODES_MAX_STEPS, native.ROUTE_CHAIN_RUN_MAX_STEPS, native.ROLLOUT_RUN_MAX_STEPS) == (256, 1024, 2048)
    assert (native.MONITOR_MAX_WINDOW, native.MONITOR_MAX_STEPS) == (1024, 4096)
    assert (native.DONE_TERMINATED, native.DONE_TRUNCATED, native.DONE_SUCCESS, native.DONE_INVALID) == (1, 2, 4, 8)
    assert (native.FLAG_PRE_NEAR_HIT, native.FLAG_NEAR_HIT, native.FLAG_SUCCESS) == (1, 2, 4)
    assert population.MAX_REPLICAS == vec_env.MAX_REPLICAS == 16
    assert native.header_int("KP1_MLP_MAX_REPLICAS") == native.header_int("KP1_CURRICULUM_MAX_REPLICAS") == native.header_int("KP1_ROUTE_MAX_REPLICAS") == 16
    assert ppo.ROUTE_FUSED_MAX_WAYPOINTS == route_curriculum.CHAIN_FUSED_MAX_WAYPOINTS == 914
    assert route_curriculum.CHAIN_RUN_MAX_STEPS == 1024
    K = mlp.MlpKernels
    assert (K.OPT_FUSED, K.OPT_ACTOR_EXTRA_STEPS, K.OPT_STEP_COUNT, K.OPT_PROFILE, K.OPT_BF16X3_WGRAD, K.OPT_TRAIN_TILE) == (1, 2, 3, 4, 5, 6)
    assert (curriculum.MAX_WINDOW, curriculum.MAX_HISTORY) == (1024, 64)
    assert (route_curriculum.MAX_STAGES, route_curriculum.MAX_WINDOW, route_curriculum.MAX_HISTORY) == (16, 1024, 32)
    assert (finisher_tools.MAX_STAGES, finisher_tools.MAX_WINDOW, finisher_tools.MAX_HISTORY) == (16, 1024, 32)


# ------------------------------------------------------------------------------------------------ struct layouts
MIRRORS = {
    "kp1_env_scalars": kcfg.EnvScalars, "kp1_approach_reward": kcfg.ApproachReward, "kp1_dock_reward": kcfg.DockReward,
    "kp1_termination": kcfg.Termination, "kp1_observation": kcfg.Observation, "kp1_stage_sampling": kcfg.StageSampling,
    "kp1_random_start": kcfg.RandomStart, "kp1_dock_reset": kcfg.DockReset, "kp1_joint_specs": kcfg.JointSpecs, "kp1_stage": kcfg.Stage,
    "kp1_config": kcfg.Kp1Config, "kp1_handoff_state": kcfg.HandoffState, "kp1_rng_state": kcfg.RngState, "kp1_reset_opts": kcfg.ResetOpts,
    "kp1_info_view": kcfg.InfoView,
    "kp1_eval_buffers": native.EvalBuffers, "kp1_route_chain_view": native.RouteChainView, "kp1_monitor_state": native.MonitorState,
    "kp1_kl_gate": native.KlGate,
    "kp1_curriculum_event": curriculum._Event, "kp1_curriculum_state": curriculum.CurriculumState,
    "kp1_route_curriculum_event": route_curriculum._CurriculumEvent, "kp1_route_curriculum_state": route_curriculum._CurriculumState,
    "kp1_route_reset_opts": route_env._RouteResetOpts, "kp1_route_info_view": route_env._RouteInfoView,
    "kp1_route_reward": route_config.RouteReward, "kp1_route_reset_cfg": route_config.RouteResetCfg, "kp1_route_config": route_config.RouteConfig,
    "kp1_dock_curriculum_stage": finisher_tools._Stage, "kp1_dock_curriculum_event": finisher_tools._Event,
    "kp1_dock_curriculum_state": finisher_tools._State,
}


def test_the_registry_of_mirrors_is_complete():
    """every ctypes.Structure the package defines is in MIRRORS (rccl's ncclUniqueId mirrors no header of this project), and every struct
    native binds by POINTER is one of them under the same C name"""
    import rl_brain_trainer_amd as pkg

    found = set()
    for path in sorted(native.PKG_DIR.glob("[!_]*.py")):
        mod = importlib.import_module(f"{pkg.__name__}.{path.stem}")
        found |= {v for v in vars(mod).values() if inspect.isclass(v) and issubclass(v, C.Structure) and v is not C.Structure}
    assert found - {rccl._UniqueId} == set(MIRRORS.values())
    assert len(MIRRORS) >= 31
    for cname, cls in native.struct_registry().items():
        assert MIRRORS[cname] is cls, cname


def test_struct_layouts_match_the_host_compiler(tmp_path):
    cc, *cc_flags = (os.environ.get("CC") or "gcc").split()
    assert shutil.which(cc), "no host C compiler ($CC or gcc): the struct layouts cannot be checked"
    lines = ["#include <stdio.h>", "#include <stddef.h>"] + [f'#include "{h}"' for h in abi.HEADERS] + ["int main(void) {"]
    for cname, cls in MIRRORS.items():
        lines.append(f'  printf("{cname} - 0 %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname} {f[0]} %zu %zu\\n", offsetof({cname}, {f[0]}), sizeof((({cname}*)0)->{f[0]}));' for f in cls._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run([cc, *cc_flags, "-std=c11", "-I", str(kcfg.repo_root() / "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    c_side = [tuple(line.split()) for line in out if line]
    py_side = []
    for cname, cls in MIRRORS.items():
        py_side.append((cname, "-", "0", str(C.sizeof(cls))))
        py_side += [(cname, f[0], str(getattr(cls, f[0]).offset), str(getattr(cls, f[0]).size)) for f in cls._fields_]
    assert len(c_side) == len(py_side) and sum(len(cls._fields_) for cls in MIRRORS.values()) >= 441
    assert [(a, b) for a, b in zip(c_side, py_side) if a != b] == []
