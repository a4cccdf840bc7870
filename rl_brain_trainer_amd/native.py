"""ctypes binding of the C ABI in include/kp1.h, kp1_ppo.h and kp1_route.h (rl_brain_trainer_amd/libkp1.so), derived from those headers:
signatures from their prototypes, constants from their defines ("The C ABI is bound from the headers").

The product path has no CPU fallback: importing this module never touches ``oracle/`` and
``load()`` raises if the HIP library has not been built (run ``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C rl_brain_trainer_amd``).
"""
from __future__ import annotations

import ctypes as C
import functools
import re
from pathlib import Path

from . import config as kcfg

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "libkp1.so"

KP1_OK = 0
REAL_F32, REAL_F64 = 0, 1
DONE_TERMINATED, DONE_TRUNCATED, DONE_SUCCESS, DONE_INVALID = 1, 2, 4, 8
FLAG_PRE_NEAR_HIT, FLAG_NEAR_HIT, FLAG_SUCCESS = 1, 2, 4


class Kp1Error(RuntimeError):
    pass


# ----------------------------------------------------------------------------- the headers are the one text of the C ABI
HEADERS = ("kp1.h", "kp1_ppo.h", "kp1_route.h")
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
# the functions whose int32_t* is a host integer (or host list) passed typed; every other int32_t* is a buffer and travels as void*
_INT32_HOST = {"kp1_get_stage", "kp1_get_reward_components", "kp1_route_curriculum_create", "kp1_route_curriculum_create_population"}
_PROTO_RE = re.compile(r"^[ \t]*((?:const\s+)?\w+[\s*]+)(kp1_\w+)\s*\(([^()]*)\)\s*;", re.M)


def strip_comments(text: str) -> str:
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


@functools.lru_cache(maxsize=None)
def header_text() -> str:
    """The three API headers, comments removed."""
    parts = []
    for name in HEADERS:
        path = kcfg.repo_root() / "include" / name
        if not path.exists():
            raise Kp1Error(f"{path} is missing: the binding is derived from the API headers")
        parts.append(strip_comments(path.read_text()))
    return "\n".join(parts)


def header_int(name: str, text: str | None = None) -> int:
    """Value of the integer ``#define name`` of the API headers: decimal, hex or ``(1 << n)``."""
    m = re.search(rf"^[ \t]*#[ \t]*define[ \t]+{re.escape(name)}[ \t]+(.*?)[ \t]*$", header_text() if text is None else strip_comments(text), flags=re.M)
    if m is None:
        raise Kp1Error(f"the API headers do not define {name}")
    shift = re.fullmatch(r"\(\s*1\s*<<\s*(\d+)\s*\)", m.group(1))
    if shift:
        return 1 << int(shift.group(1))
    if not re.fullmatch(r"\d+|0[xX][0-9a-fA-F]+", m.group(1)):
        raise Kp1Error(f"#define {name} {m.group(1)}: not a decimal, hex or (1 << n) integer")
    return int(m.group(1), 0)


def _ctype(func: str, decl: str, structs: dict, ret: bool = False):
    words = decl.replace("*", " * ").split()
    stars = words.count("*")
    words = [w for w in words if w not in ("const", "struct", "*")]    # what is left: the type, then the parameter's name if it has one
    base = words[0] if words else ""
    if "[" not in decl and 1 <= len(words) <= (1 if ret else 2):
        if stars == 0 and base in _SCALARS:
            return _SCALARS[base]
        if stars == 0 and ret and base == "void":
            return None
        if stars == 1 and ret and base == "char":
            return C.c_char_p
        if stars == 1 and not ret:
            if base in structs and not words[-1].endswith("_dev"):      # the headers' *_dev parameters are device memory: a handle, never a mirror
                return C.POINTER(structs[base])
            return C.POINTER(C.c_int32) if base == "int32_t" and func in _INT32_HOST else C.c_void_p
        if stars == 2 and not ret:
            return C.POINTER(C.c_void_p)
    raise Kp1Error(f"{func}: no ctypes type for {'return type' if ret else 'parameter'} '{' '.join(decl.split())}'")


def parse_prototypes(text: str, structs: dict) -> dict[str, tuple]:
    """{name: (restype, [argtypes])} of every ``kp1_*`` function declaration in ``text`` (C, comments allowed)."""
    out = {}
    for ret, name, params in _PROTO_RE.findall(strip_comments(text)):
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (_ctype(name, ret, structs, ret=True), [_ctype(name, p, structs) for p in params])
    return out


def declared_symbols() -> list[str]:
    """Every function the API headers declare."""
    return [name for _, name, _ in _PROTO_RE.findall(header_text())]


EVAL_EPISODES_MAX_STEPS = header_int("KP1_EVAL_EPISODES_MAX_STEPS")          # env steps of one kp1_eval_episodes call
ROUTE_CHAIN_RUN_MAX_STEPS = header_int("KP1_ROUTE_CHAIN_RUN_MAX_STEPS")      # lock steps of one kp1_route_chain_run call
ROLLOUT_RUN_MAX_STEPS = header_int("KP1_ROLLOUT_RUN_MAX_STEPS")              # env steps of one kp1_rollout_run call
MONITOR_MAX_WINDOW = header_int("KP1_MONITOR_MAX_WINDOW")
MONITOR_MAX_STEPS = header_int("KP1_MONITOR_MAX_STEPS")


class EvalBuffers(C.Structure):
    """include/kp1.h kp1_eval_buffers: device pointers of the batched evaluator's per-episode accumulators"""
    _fields_ = [(n, C.c_void_p) for n in ("metrics", "counters", "flags", "state", "hand_metrics", "hand_step", "hand_success", "hand_state", "n_alive")]


class RouteChainView(C.Structure):
    """include/kp1_route.h kp1_route_chain_view: device pointers of a chain's record table and counters"""
    _fields_ = [("records", C.c_void_p), ("n_records", C.c_void_p), ("n_alive", C.c_void_p), ("n_rows", C.c_int32), ("max_len", C.c_int32)]


class MonitorState(C.Structure):
    """include/kp1_ppo.h kp1_monitor_state: one replica's ring of the newest `window` episodes and its totals"""
    _fields_ = [("window", C.c_int32), ("ring_len", C.c_int32), ("ring_head", C.c_int32), ("reserved0", C.c_int32),
                ("total_episodes", C.c_int64), ("total_successes", C.c_int64),
                ("ring_return", C.c_double * MONITOR_MAX_WINDOW), ("ring_length", C.c_int32 * MONITOR_MAX_WINDOW),
                ("ring_success", C.c_uint8 * MONITOR_MAX_WINDOW)]


class KlGate(C.Structure):
    """include/kp1_ppo.h kp1_kl_gate: one replica's KL early-stop record (SB3 PPO's target_kl as a device decision)"""
    _fields_ = [("threshold", C.c_double), ("stopped", C.c_int32), ("n_counted", C.c_int32), ("n_seen", C.c_int32), ("stop_index", C.c_int32),
                ("stop_kl", C.c_float), ("reserved0", C.c_int32)]


def struct_registry() -> dict[str, type[C.Structure]]:
    """C struct name -> ctypes mirror of every struct a function takes by pointer from a host caller that builds the mirror; a parameter
    of such a type binds as ``POINTER(mirror)``.  (The modules that own the route and curriculum mirrors import this one, hence the late import.)"""
    from . import finisher_tools, route_config, route_curriculum, route_env

    return {"kp1_config": kcfg.Kp1Config, "kp1_reset_opts": kcfg.ResetOpts, "kp1_info_view": kcfg.InfoView, "kp1_rng_state": kcfg.RngState,
            "kp1_eval_buffers": EvalBuffers, "kp1_route_chain_view": RouteChainView, "kp1_monitor_state": MonitorState,
            "kp1_route_config": route_config.RouteConfig, "kp1_route_reset_opts": route_env._RouteResetOpts,
            "kp1_route_info_view": route_env._RouteInfoView, "kp1_route_curriculum_state": route_curriculum._CurriculumState,
            "kp1_dock_curriculum_stage": finisher_tools._Stage, "kp1_dock_curriculum_state": finisher_tools._State}


_lib: C.CDLL | None = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise Kp1Error(
            f"{LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback; "
            "build it with `python -c 'import __graft_entry__ as g; g.build()'`."
        )
    L = C.CDLL(str(LIB_PATH))
    for name, (restype, argtypes) in parse_prototypes(header_text(), struct_registry()).items():
        if not hasattr(L, name):
            raise Kp1Error(f"{LIB_PATH} does not export {name}, which the API headers declare")
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.kp1_config_size() != C.sizeof(kcfg.Kp1Config):
        raise Kp1Error(f"kp1_config layout mismatch: library {L.kp1_config_size()} vs binding {C.sizeof(kcfg.Kp1Config)}")
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != KP1_OK:
        msg = load().kp1_last_error().decode(errors="replace")
        if rc == -1:
            raise ValueError(msg)
        raise Kp1Error(f"kp1 error {rc}: {msg}")


def ptr(t):
    """a tensor's device address as the ``void*`` argument of a C entry point; None (NULL) for None"""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_arg(device) -> C.c_void_p:
    """the current stream of ``device`` as the ``stream`` argument of a C entry point (torch is imported here: this module needs none)"""
    import torch

    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def device_index(device) -> int:
    """the ``device`` argument of a C entry point: a torch device's ordinal, 0 where it carries none"""
    return device.index or 0


def component_names(mode: int) -> list[str]:
    L = load()
    return [L.kp1_component_name(mode, i).decode() for i in range(L.kp1_num_components(mode))]
