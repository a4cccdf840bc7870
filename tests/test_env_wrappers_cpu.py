"""The Python half of the env handles without a device: ``ArmKinematicVecEnv``, ``ArmKinematicPopulationVecEnv``,
``RouteVecEnv``, ``RoutePopulationVecEnv``, their replica views and ``RouteChain`` stood on CPU tensors over a recording library, and the
exact sequence of library calls, with their arguments, that every public method makes.

How the handles stand here.  ``native.load`` gives ``_Lib``: every ``kp1_*`` call is recorded and returns 0; the create calls write a
handle through their ``out`` pointer, ``kp1_route_obs_dim`` answers 80, and the calls that fill host memory (``*_rng_get``,
``kp1_get_state``, ``kp1_route_get_dataset``, the info views) fill it with distinct values.  ``torch.cuda.is_available`` answers True,
``torch.cuda.device`` is a null context, ``torch.cuda.current_stream`` a stub with a known address, and ``_view`` in both modules
returns a tagged tuple instead of wrapping a device pointer.

How calls are compared.  Scalars by value; ``None`` as ``None``; a pointer as the name of the buffer it points to (``_Lib.take`` maps
``data_ptr`` -> name over the handle's own buffers and the test's), or, where the wrapper made the buffer itself (a cast action, a
broadcast option row), as the values the library would read there; a struct passed by reference as its bytes, or, for the reset options,
as the fields the method set.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden_config
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import route_config as rcfg
from rl_brain_trainer_amd import route_env as re_
from rl_brain_trainer_amd import vec_env as ve

CPU = torch.device("cpu")
STREAM = 0x5150
NJ = kcfg.NJ
ARG = type(C.byref(C.c_int()))
STATE_KEYS = (("q", 7), ("dq", 7), ("prev_action", 7), ("goal_q", 7), ("goal_pose6", 6))
RESET_KEYS = (("initial_q", 7), ("initial_dq", 7), ("initial_prev_action", 7), ("goal_q", 7), ("goal_pose6", 6))


class _Ptr:
    """a pointer argument as it was at the call: resolved to a buffer name by ``_Lib.take``, else to the values read at the call"""

    def __init__(self, addr: int, values=None) -> None:
        self.addr, self.values = int(addr), values


def _addr(a) -> int | None:
    if a is None:
        return None
    return a.value if isinstance(a, C.c_void_p) else int(a)


def _read(a, ctype, count: int) -> tuple:
    addr = _addr(a)
    return None if addr is None else tuple((ctype * count).from_address(addr))


def _rows(a, n: int, w: int, ctype=C.c_double):
    flat = _read(a, ctype, n * w)
    return None if flat is None else tuple(flat[i * w:(i + 1) * w] for i in range(n))


def _fill(a, values: np.ndarray) -> None:
    addr = _addr(a)
    if addr is not None:
        C.memmove(addr, np.ascontiguousarray(values).ctypes.data, values.nbytes)


def state_values(n: int) -> dict[str, np.ndarray]:
    """what the recording kp1_get_state writes"""
    return {k: 1000.0 * (j + 1) + np.arange(n * w, dtype=np.float64).reshape(n, w) for j, (k, w) in enumerate(STATE_KEYS)}


def rng_words(n: int, salt: int) -> np.ndarray:
    """what the recording *_rng_get writes: all six words distinct, state_hi above 2**63"""
    w = np.zeros((n, 6), dtype=np.uint64)
    for i in range(n):
        w[i] = [2**63 + 1000 * salt + i, 2**40 + i, 77 + i, 2 * i + 1, i % 2, 0xFFFF0000 + i]
    return w


def dataset_values(W: int) -> dict[str, np.ndarray]:
    """what the recording kp1_route_get_dataset writes"""
    return {"poses6": 0.5 + np.arange(W * 6, dtype=np.float64).reshape(W, 6), "route_progress_m": 0.25 * np.arange(W, dtype=np.float64),
            "next_q_delta": -1.0 - np.arange(W * NJ, dtype=np.float64).reshape(W, NJ), "chunk_id": (np.arange(W) // 3).astype(np.int32)}


class _Lib:
    """the recording library"""

    def __init__(self) -> None:
        self.calls: list[tuple] = []
        self.n = 0                   # rows of the handle under test (what the hooks read behind a pointer)
        self.f64 = False
        self.obs_dim = 80
        self.n_handles = 0
        self.W = 0

    def __getattr__(self, name: str):
        if not name.startswith("kp1_"):
            raise AttributeError(name)

        def call(*args):
            hook = getattr(self, "_" + name, None)
            out = hook(*args) if hook is not None else (None, 0)
            items, ret = out if isinstance(out, tuple) else (out, 0)
            self.calls.append((name, [self._item(a) for a in args] if items is None else items))
            return ret

        return call

    @staticmethod
    def _item(a):
        if a is None or isinstance(a, (bool, int, float)):
            return a
        if isinstance(a, C.c_void_p):
            return _Ptr(a.value or 0)
        if isinstance(a, ARG):
            return (type(a._obj).__name__, bytes(a._obj))
        raise AssertionError(f"no rule for argument {a!r}")

    def take(self, env=None, **buffers) -> list[tuple]:
        """the calls since the last take(), pointers resolved to names over ``env``'s own buffers and ``buffers``"""
        names = {STREAM: "stream"}
        if env is not None:
            for key in ("obs", "terminal_obs", "reward", "done"):
                names[getattr(env, key).data_ptr()] = key
            if getattr(env, "_handle", None) is not None and env._handle.value:
                names[env._handle.value] = "handle"
            base = getattr(env, "base", None)
            if base is not None and base._handle.value:
                names[base._handle.value] = "base_handle"
            if hasattr(env, "route_q"):
                names[env.route_q.ctypes.data] = "route_q"
        for key, buf in buffers.items():
            names[buf if isinstance(buf, int) else buf.data_ptr() if isinstance(buf, torch.Tensor) else buf.ctypes.data] = key
        out = []
        for name, items in self.calls:
            out.append((name, *[(names.get(i.addr, ("values", i.values)) if i.addr else None) if isinstance(i, _Ptr) else i for i in items]))
        self.calls = []
        return out

    def _new_handle(self, out) -> str:
        self.n_handles += 1
        out._obj.value = 0xA000 + 0x100 * self.n_handles
        return "out"

    # ---- arm
    def _kp1_create(self, cfg, n, dev, real, seed, first, stream, out):
        return [self._item(cfg), n, dev, real, seed, first, self._item(stream), self._new_handle(out)]

    def _kp1_set_handoff_states(self, h, arr, count):
        return [self._item(h), bytes((kcfg.HandoffState * max(count, 1)).from_address(_addr(arr))), count]

    def _kp1_set_route_stride_reset(self, h, q, nq, lo, nlo, hi, nhi, sn, gn, prob):
        return [self._item(h), _rows(q, nq, NJ), nq, _read(lo, C.c_int32, nlo), nlo, _read(hi, C.c_int32, nhi), nhi, _read(sn, C.c_double, NJ),
                _read(gn, C.c_double, NJ), prob]

    def _kp1_seed_blocks(self, h, seeds, K, n):
        return [self._item(h), _read(seeds, C.c_uint64, K), K, n]

    def _mask(self, mask):
        return None if mask is None else _Ptr(mask.value, _read(mask, C.c_uint8, self.n))

    def _kp1_reset(self, h, mask, opts, obs):
        o = None
        if opts is not None:
            o = {key: _rows(getattr(opts._obj, key), self.n, w) for key, w in RESET_KEYS}
            o["policy_mode"] = opts._obj.policy_mode
        return [self._item(h), self._mask(mask), o, self._item(obs)]

    def _actions(self, a):
        return _Ptr(a.value, _rows(a, self.n, NJ, C.c_double if self.f64 else C.c_float))

    def _kp1_step(self, h, a, *rest):
        return [self._item(h), self._actions(a)] + [self._item(r) for r in rest]

    _kp1_route_step = _kp1_step

    def _kp1_get_stage(self, h, out):
        out._obj.value = 3
        return [self._item(h), "out"]

    def _info(self, h, view):
        for j, (name, ctype) in enumerate(type(view._obj)._fields_):
            setattr(view._obj, name, 0x100000 + 0x100 * j if ctype is C.c_void_p else 0)
        return [self._item(h), "out"]

    _kp1_get_info = _kp1_route_get_info = _info

    def _kp1_get_reward_components(self, h, ptr, n):
        ptr._obj.value, n._obj.value = 0x7700, 5
        return [self._item(h), "out", "out"]

    def _kp1_route_get_reward_components(self, h, ptr):
        ptr._obj.value = 0x7800
        return [self._item(h), "out"]

    def _kp1_num_components(self, mode):
        return None, 2

    def _kp1_component_name(self, mode, i):
        return None, f"component_{mode}_{i}".encode()

    def _kp1_get_state(self, h, *ptrs):
        for p, (key, _w) in zip(ptrs, STATE_KEYS):
            _fill(p, state_values(self.n)[key])
        return [self._item(h)] + ["out" if p is not None else None for p in ptrs]

    def _kp1_set_state(self, h, *rest):
        return [self._item(h)] + [_rows(p, self.n, w) for p, (_k, w) in zip(rest, STATE_KEYS)] + [rest[5]]

    def _rng_get(self, salt):
        def hook(h, arr):
            words = rng_words(self.n, salt)
            for i in range(self.n):
                (arr[i].state_hi, arr[i].state_lo, arr[i].inc_hi, arr[i].inc_lo, arr[i].has_uint32, arr[i].uinteger) = (int(v) for v in words[i])
            return [self._item(h), "out"]
        return hook

    _kp1_rng_get = property(lambda self: self._rng_get(1))
    _kp1_route_rng_get = property(lambda self: self._rng_get(2))

    def _kp1_rng_set(self, h, arr):
        assert len(arr) == self.n
        return [self._item(h), tuple((s.state_hi, s.state_lo, s.inc_hi, s.inc_lo, s.has_uint32, s.uinteger) for s in arr)]

    _kp1_route_rng_set = _kp1_rng_set

    # ---- route
    def _kp1_route_create(self, base, cfg, q, W, seed, first, out):
        self.W = W
        return [self._item(base), self._item(cfg), self._item(q), W, seed, first, self._new_handle(out)]

    def _kp1_route_create_population(self, base, cfg, q, W, seeds, K, out):
        self.W = W
        return [self._item(base), self._item(cfg), self._item(q), W, _read(seeds, C.c_uint64, K), K, self._new_handle(out)]

    def _kp1_route_obs_dim(self, h):
        return None, self.obs_dim

    def _kp1_route_get_dataset(self, h, *ptrs):
        for p, values in zip(ptrs, dataset_values(self.W).values()):
            _fill(p, values)
        return [self._item(h), "out", "out", "out", "out"]

    def _kp1_route_reset(self, h, mask, opts, obs):
        o = None
        if opts is not None:
            s = opts._obj
            o = {"route_index": _read(s.route_index, C.c_int32, self.n), "start_route_index": _read(s.start_route_index, C.c_int32, self.n),
                 **{key: _rows(getattr(s, key), self.n, NJ) for key in ("initial_q", "initial_dq", "initial_prev_action")},
                 "evaluator_state": s.evaluator_state}
            self.route_reset_ptrs = [p for p in (s.route_index, s.start_route_index, s.initial_q, s.initial_dq, s.initial_prev_action) if p]
        return [self._item(h), self._mask(mask), o, self._item(obs)]

    def _kp1_route_chain_create(self, h, start, end, n, stop, out):
        out._obj.value = 0xC000
        return [self._item(h), _read(start, C.c_int32, n), _read(end, C.c_int32, n), n, stop, "out"]

    def _kp1_route_chain_get_view(self, h, view):
        view._obj.records, view._obj.n_records, view._obj.n_alive, view._obj.n_rows, view._obj.max_len = 0x200000, 0x200100, 0x200200, self.n, 4
        return [self._item(h), "out"]


@pytest.fixture
def lib(monkeypatch):
    fake = _Lib()
    monkeypatch.setattr(native, "load", lambda: fake)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device", lambda _d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda _d=None: types.SimpleNamespace(cuda_stream=STREAM))
    for mod in (ve, re_):
        monkeypatch.setattr(mod, "_view", lambda ptr, shape, typestr, device: ("view", ptr, tuple(shape), typestr, device))
    return fake


def cfg_item(c) -> tuple:
    return (type(c).__name__, bytes(c))


def _arm(lib, n=8, cfg=None, **kw):
    cfg = cfg or load_golden_config("approach_default")
    lib.n, lib.f64 = n, kw.get("real") == "f64"
    return ve.ArmKinematicVecEnv(cfg, n, device=CPU, **kw), cfg


def _route_parts():
    cfgd = json.loads((GOLDEN / "configs" / "route_curriculum_prefix120_routeobs_sequence2.json").read_text())
    return kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=40), rcfg.load_route_q(GOLDEN / "synthetic_route.json")


def _route(lib, n=6, **kw):
    base_cfg, route_cfg, route_q = _route_parts()
    lib.n, lib.f64 = n, kw.get("real") == "f64"
    return re_.RouteVecEnv(base_cfg, route_cfg, route_q, n, device=CPU, **kw), base_cfg, route_cfg


def _arm_pop(lib, seeds=(11, 2**32 + 5), n_per=4, cfg=None, **kw):
    cfg = cfg or load_golden_config("approach_default")
    lib.n, lib.f64 = len(seeds) * n_per, False
    return ve.ArmKinematicPopulationVecEnv(cfg, list(seeds), n_per, device=CPU, **kw), cfg


def _route_pop(lib, seeds=(11, 2**32 + 5, 40), n_per=2, **kw):
    base_cfg, route_cfg, route_q = _route_parts()
    lib.n, lib.f64 = len(seeds) * n_per, False
    return re_.RoutePopulationVecEnv(base_cfg, route_cfg, route_q, list(seeds), n_per, device=CPU, **kw), base_cfg, route_cfg


# ------------------------------------------------------------------------------------------------------------------------ constructors
def test_arm_constructor(lib):
    env, cfg = _arm(lib, n=8, seed=5, first_env_id=2)
    assert lib.take(env) == [("kp1_create", cfg_item(cfg.c), 8, 0, native.REAL_F32, 5, 2, "stream", "out")]
    assert env._handle.value and env.n_envs == 8 and env.device == CPU and env.dtype == torch.float32 and env.real_type == native.REAL_F32
    assert env.obs.shape == env.terminal_obs.shape == (8, 56) and env.obs.dtype == env.terminal_obs.dtype == torch.float32
    assert env.reward.shape == (8,) and env.reward.dtype == torch.float32 and env.done.shape == (8,) and env.done.dtype == torch.uint8
    assert env.obs_stride == 56 and env.launch_args_version == 0 and env._mode_name == "approach" and not hasattr(env, "obs_dim")
    assert not hasattr(env, "is_population") and not hasattr(env, "_reward_components_on")

    env64, _ = _arm(lib, n=3, real="f64", reward_components=True)
    assert lib.take(env64) == [("kp1_create", cfg_item(cfg.c), 3, 0, native.REAL_F64, 0, 0, "stream", "out"),
                               ("kp1_enable_reward_components", "handle", 1)]
    assert env64.dtype == env64.reward.dtype == torch.float64 and env64.obs.dtype == torch.float32
    assert env64._reward_components_on is True and env64.launch_args_version == 1


def test_arm_constructor_handoff_states_and_route_reset(lib):
    dock = load_golden_config("dock_workspace_handoff_noop_ft_12env_raw")
    dock.handoff_states = dock.handoff_states[:3]
    dock_env, _ = _arm(lib, n=4, cfg=dock, seed=9)
    assert lib.take(dock_env) == [("kp1_create", cfg_item(dock.c), 4, 0, native.REAL_F32, 9, 0, "stream", "out"),
                                  ("kp1_set_handoff_states", "handle", bytes(dock.handoff_array()), 3)]
    assert dock_env._mode_name == "dock" and dock_env.launch_args_version == 0

    cfg = load_golden_config("approach_default")
    pts = tuple(tuple(0.01 * (i + 1) * (j + 1) for j in range(NJ)) for i in range(5))
    rr = kcfg.RouteResetConfig(enabled=True, route_q=pts, min_stride_by_stage=(1, 2), max_stride_by_stage=(2, 3, 4), start_q_noise=(0.01,) * NJ,
                               goal_q_noise=(0.02,) * NJ, reverse_probability=0.25)
    cfg.route_reset = rr
    env, _ = _arm(lib, n=4, cfg=cfg)
    stride_call = ("kp1_set_route_stride_reset", "handle", pts, 5, (1, 2), 2, (2, 3, 4), 3, (0.01,) * NJ, (0.02,) * NJ, 0.25)
    assert lib.take(env) == [("kp1_create", cfg_item(cfg.c), 4, 0, native.REAL_F32, 0, 0, "stream", "out"), stride_call]
    assert env.config.route_reset is rr and env.launch_args_version == 0
    env.set_route_stride_reset(None)
    assert lib.take(env) == [("kp1_set_route_stride_reset", "handle", None, 0, None, 0, None, 0, None, None, 0.0)]
    assert env.config.route_reset == kcfg.RouteResetConfig() and env.launch_args_version == 0
    env.set_route_stride_reset(rr)
    assert lib.take(env) == [stride_call]


def _dataset_filled(env) -> bool:
    want = dataset_values(env.n_waypoints)
    return all(np.array_equal(getattr(env, key), want[key]) and getattr(env, key).dtype == want[key].dtype for key in want)


def test_route_constructor(lib):
    env, base_cfg, route_cfg = _route(lib, n=6, seed=5, first_env_id=2)
    W = env.n_waypoints
    assert lib.take(env) == [("kp1_create", cfg_item(base_cfg.c), 6, 0, native.REAL_F32, 5, 2, "stream", "out"),
                             ("kp1_route_create", "base_handle", cfg_item(route_cfg), "route_q", W, 5, 2, "out"),
                             ("kp1_route_obs_dim", "handle"),
                             ("kp1_route_get_dataset", "handle", "out", "out", "out", "out")]
    assert type(env.base) is ve.ArmKinematicVecEnv and env.base._handle.value != env._handle.value and env.L is env.base.L
    assert env.config is base_cfg and env.route_cfg is route_cfg and env.route_q.shape == (W, NJ) and env.route_q.dtype == np.float64
    assert env.n_envs == 6 and env.device == CPU and env.dtype == torch.float32 and env.obs_dim == env.obs_stride == 80
    assert env.obs.shape == env.terminal_obs.shape == (6, 80) and env.obs.dtype == torch.float32
    assert env.reward.shape == (6,) and env.reward.dtype == torch.float32 and env.done.dtype == torch.uint8
    assert _dataset_filled(env)                         # the four host arrays the handle keeps are the ones the library filled
    assert env.launch_args_version == 0 and env._reward_components_on is False and not hasattr(env, "is_population")

    env64, _, _ = _route(lib, n=2, real="f64", reward_components=True)
    calls = lib.take(env64)
    assert calls[0][4] == native.REAL_F64 and calls[-1] == ("kp1_route_enable_reward_components", "handle", 1) and len(calls) == 5
    assert env64.reward.dtype == torch.float64 and env64._reward_components_on is True and env64.launch_args_version == 1

    with pytest.raises(ValueError, match=r"route_q must have shape \(n_waypoints, 7\)"):
        re_.RouteVecEnv(base_cfg, route_cfg, np.zeros((4, 6)), 2, device=CPU)


def test_route_obs_dim_56(lib):
    lib.obs_dim = 56
    env, _, _ = _route(lib, n=2)
    assert env.obs_dim == env.obs_stride == 56 and env.obs.shape == (2, 56)


def test_arm_population_constructor(lib):
    pop, cfg = _arm_pop(lib, seeds=(11, 2**32 + 5), n_per=4, reward_components=True)
    assert lib.take(pop) == [("kp1_create", cfg_item(cfg.c), 8, 0, native.REAL_F32, 11, 0, "stream", "out"),
                             ("kp1_enable_reward_components", "handle", 1),
                             ("kp1_seed_blocks", "handle", (11, 2**32 + 5), 2, 4)]
    assert pop.seeds == [11, 2**32 + 5] and pop.K == 2 and pop.n_per_replica == 4 and pop.n_envs == 8 and pop.is_population is True
    assert pop.dock_population is None and pop.rows(1) == slice(4, 8) and pop.obs.shape == (8, 56)
    same, _ = _arm_pop(lib, seeds=(7, 7), n_per=1, repeated_seeds=True)
    assert lib.take(same)[-1] == ("kp1_seed_blocks", "handle", (7, 7), 2, 1)
    with pytest.raises(ValueError, match="n_per_replica must be positive"):
        _arm_pop(lib, n_per=0)
    assert lib.take() == []


def test_route_population_constructor(lib):
    pop, base_cfg, route_cfg = _route_pop(lib, seeds=(11, 2**32 + 5, 40), n_per=2, reward_components=True)
    W = pop.n_waypoints
    assert lib.take(pop) == [("kp1_create", cfg_item(base_cfg.c), 6, 0, native.REAL_F32, 11, 0, "stream", "out"),
                             ("kp1_route_create_population", "base_handle", cfg_item(route_cfg), "route_q", W, (11, 2**32 + 5, 40), 3, "out"),
                             ("kp1_route_obs_dim", "handle"),
                             ("kp1_route_get_dataset", "handle", "out", "out", "out", "out"),
                             ("kp1_route_enable_reward_components", "handle", 1)]
    assert pop.seeds == [11, 2**32 + 5, 40] and pop.K == 3 and pop.n_per_replica == 2 and pop.n_envs == 6 and not hasattr(pop, "is_population")
    assert pop.rows(2) == slice(4, 6) and [pop.window(k) for k in range(3)] == [(int(route_cfg.reset.min_route_index), int(route_cfg.reset.max_route_index))] * 3
    assert _dataset_filled(pop)
    for seeds, n_per, match in (([], 2, "RoutePopulationVecEnv needs at least one seed"), ([1], 0, "n_per_replica must be positive")):
        with pytest.raises(ValueError, match=match):
            re_.RoutePopulationVecEnv(base_cfg, route_cfg, pop.route_q, seeds, n_per, device=CPU)
    assert lib.take() == []


def test_no_device_is_refused(lib, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(native.Kp1Error, match="ArmKinematicVecEnv needs a HIP device"):
        ve.ArmKinematicVecEnv(load_golden_config("approach_default"), 2, device=CPU)
    assert lib.take() == []


# ------------------------------------------------------------------------------------------------------------------------ reset
def _full(row, n):
    return tuple(tuple(float(v) for v in row) for _ in range(n))


def test_arm_reset(lib):
    env, _ = _arm(lib, n=4)
    lib.take()
    assert env.reset() is env.obs
    assert lib.take(env) == [("kp1_reset", "handle", None, None, "obs")]
    assert env.reset(seed=31) is env.obs
    assert lib.take(env) == [("kp1_seed", "handle", 31, 0), ("kp1_reset", "handle", None, None, "obs")]
    none = {key: None for key, _ in RESET_KEYS}
    rng = np.random.default_rng(0)
    for key, w in RESET_KEYS:
        mat = rng.normal(size=(4, w))
        env.reset(options={key: mat})
        assert lib.take(env) == [("kp1_reset", "handle", None, {**none, key: tuple(map(tuple, mat.tolist())), "policy_mode": -1}, "obs")]
        env.reset(options={key: mat[1].astype(np.float32)})          # one row, broadcast; any dtype that casts to float64
        assert lib.take(env) == [("kp1_reset", "handle", None, {**none, key: _full(mat[1].astype(np.float32), 4), "policy_mode": -1}, "obs")]
        for bad in (np.zeros((3, w)), np.zeros(w + 1), np.zeros((4, w, 1))):
            with pytest.raises(ValueError, match=rf"options\['{key}'\] must have shape \(4, {w}\), got "):
                env.reset(options={key: bad})
        assert lib.take() == []
    q, g = rng.normal(size=(4, 7)), rng.normal(size=6)
    env.reset(options={"goal_pose6": g, "initial_q": q, "policy_mode": "dock"})
    assert lib.take(env) == [("kp1_reset", "handle", None, {**none, "initial_q": tuple(map(tuple, q.tolist())), "goal_pose6": _full(g, 4), "policy_mode": 1},
                              "obs")]
    assert env._mode_name == "dock"
    env.reset(options={"initial_q": q})                               # options without a mode keep the last reset's mode name
    assert env._mode_name == "dock" and lib.take(env)[0][3]["policy_mode"] == -1
    env.reset()                                                       # no options: back to the config's mode
    assert env._mode_name == "approach"
    with pytest.raises(ValueError, match="Unsupported policy mode 'bridge'"):
        env.reset(options={"policy_mode": "bridge"})
    lib.take()
    mask = torch.tensor([1, 0, 0, 1], dtype=torch.uint8)
    env.reset(mask=mask)
    assert lib.take(env, mask=mask) == [("kp1_reset", "handle", "mask", None, "obs")]
    env.reset(mask=torch.tensor([True, False, True, True]))          # cast to bytes first
    assert lib.take(env) == [("kp1_reset", "handle", ("values", (1, 0, 1, 1)), None, "obs")]
    assert env.launch_args_version == 0


def test_route_reset(lib):
    env, _, _ = _route(lib, n=3)
    lib.take()
    assert env.reset() is env.obs and env._keep == []
    assert lib.take(env) == [("kp1_route_reset", "handle", None, None, "obs")]
    env.reset(seed=8)
    assert lib.take(env) == [("kp1_route_seed", "handle", 8, 0), ("kp1_route_reset", "handle", None, None, "obs")]
    env.reset(options={"start_route_index": 4})                       # without route_index the options are not read
    assert lib.take(env) == [("kp1_route_reset", "handle", None, None, "obs")]
    none = {key: None for key in ("start_route_index", "initial_q", "initial_dq", "initial_prev_action")}
    env.reset(options={"route_index": 7})
    assert lib.take(env) == [("kp1_route_reset", "handle", None, {"route_index": (7, 7, 7), **none, "evaluator_state": 0}, "obs")]
    assert [t.data_ptr() for t in env._keep] == lib.route_reset_ptrs and len(env._keep) == 1
    rng = np.random.default_rng(1)
    q, dq, pa = rng.normal(size=(3, 7)), rng.normal(size=7), rng.normal(size=(3, 7))
    mask = torch.tensor([0, 1, 1], dtype=torch.uint8)
    env.reset(options={"route_index": [5, 6, 7], "start_route_index": np.array([1, 2, 3]), "initial_q": q, "initial_dq": dq, "initial_prev_action": pa,
                       "evaluator_state": True}, mask=mask)
    want = {"route_index": (5, 6, 7), "start_route_index": (1, 2, 3), "initial_q": tuple(map(tuple, q.tolist())), "initial_dq": _full(dq, 3),
            "initial_prev_action": tuple(map(tuple, pa.tolist())), "evaluator_state": 1}
    assert lib.take(env, mask=mask) == [("kp1_route_reset", "handle", "mask", want, "obs")]
    # the device copies (and the mask) stay alive until the next reset
    assert [t.data_ptr() for t in env._keep[:5]] == lib.route_reset_ptrs and env._keep[5] is mask and len(env._keep) == 6
    env.reset(mask=torch.tensor([True, False, True]))
    assert lib.take(env) == [("kp1_route_reset", "handle", ("values", (1, 0, 1)), None, "obs")]
    assert len(env._keep) == 1 and env._keep[0].dtype == torch.uint8
    assert env.launch_args_version == 0


# ------------------------------------------------------------------------------------------------------------------------ stepping
def _caller_buffers(n, w, dtype=torch.float32):
    return {"c_act": torch.rand(n, NJ, dtype=dtype), "c_obs": torch.zeros(n, w), "c_rew": torch.zeros(n, dtype=dtype),
            "c_done": torch.zeros(n, dtype=torch.uint8), "c_term": torch.zeros(n, w)}


@pytest.mark.parametrize("family, real", [("arm", "f32"), ("arm", "f64"), ("route", "f32"), ("route", "f64"), ("arm_pop", "f32"), ("route_pop", "f32")])
def test_step_and_step_into(lib, family, real):
    env = {"arm": lambda: _arm(lib, n=4, real=real), "route": lambda: _route(lib, n=4, real=real), "arm_pop": lambda: _arm_pop(lib, n_per=2),
           "route_pop": lambda: _route_pop(lib, seeds=(1, 2), n_per=2)}[family]()[0]
    lib.take()
    call = "kp1_route_step" if family.startswith("route") else "kp1_step"
    b = _caller_buffers(4, 128, env.dtype)
    a = b["c_act"]
    assert env.step(a) == (env.obs, env.reward, env.done) and env.step(a)[0] is env.obs
    assert lib.take(env, **b) == [(call, "handle", "c_act", "obs", "reward", "done", "terminal_obs", 1)] * 2
    env.step(a, auto_reset=False)
    assert lib.take(env, **b) == [(call, "handle", "c_act", "obs", "reward", "done", "terminal_obs", 0)]
    other = torch.float64 if env.dtype == torch.float32 else torch.float32
    env.step(a.to(other))                                             # cast to the env's real type first
    cast = tuple(map(tuple, a.to(other).to(env.dtype).tolist()))
    assert lib.take(env, **b) == [(call, "handle", ("values", cast), "obs", "reward", "done", "terminal_obs", 1)]
    env.step(a.T.contiguous().T)                                      # made contiguous first
    assert lib.take(env, **b) == [(call, "handle", ("values", tuple(map(tuple, a.tolist()))), "obs", "reward", "done", "terminal_obs", 1)]
    for bad in (torch.zeros(3, NJ), torch.zeros(4, 6), torch.zeros(4 * NJ)):
        with pytest.raises(ValueError, match=r"Expected action shape \(4, 7\), got \(" + ", ".join(str(s) for s in bad.shape)):
            env.step(bad)
    assert env.step_into(a, b["c_obs"], b["c_rew"], b["c_done"], b["c_term"]) is None
    env.step_into(a, b["c_obs"], b["c_rew"], b["c_done"], None)
    env.step_into(a, b["c_obs"], b["c_rew"], b["c_done"], b["c_term"], False)
    env.step_into(a, b["c_obs"], b["c_rew"], b["c_done"], None, auto_reset=False)
    assert lib.take(env, **b) == [(call, "handle", "c_act", "c_obs", "c_rew", "c_done", "c_term", 1), (call, "handle", "c_act", "c_obs", "c_rew", "c_done", None, 1),
                                  (call, "handle", "c_act", "c_obs", "c_rew", "c_done", "c_term", 0), (call, "handle", "c_act", "c_obs", "c_rew", "c_done", None, 0)]
    assert env.launch_args_version == 0


def test_set_obs_stride_and_use_current_stream(lib):
    arm, _ = _arm(lib, n=4, real="f64")
    route, _, _ = _route(lib, n=4)
    lib.take()
    old = arm.obs
    arm.set_obs_stride(64)
    assert lib.take(arm) == [("kp1_set_obs_stride", "handle", 64)]
    assert arm.obs is not old and arm.obs.shape == arm.terminal_obs.shape == (4, 64) and arm.obs.dtype == arm.terminal_obs.dtype == torch.float32
    assert arm.obs.data_ptr() != arm.terminal_obs.data_ptr() and not arm.obs.any() and not arm.terminal_obs.any()
    assert arm.obs_stride == 64 and arm.launch_args_version == 1 and arm.reward.dtype == torch.float64
    arm.set_obs_stride(64)                                            # the handle itself forwards every call
    assert lib.take(arm) == [("kp1_set_obs_stride", "handle", 64)] and arm.launch_args_version == 2
    route.set_obs_stride(128)
    assert lib.take(route) == [("kp1_route_set_obs_stride", "handle", 128)]
    assert route.obs.shape == route.terminal_obs.shape == (4, 128) and route.obs.data_ptr() != route.terminal_obs.data_ptr()
    assert route.obs_stride == 128 and route.obs_dim == 80 and route.launch_args_version == 0       # the route handle does not bump
    assert route.base.obs_stride == 56 and route.base.launch_args_version == 0
    arm.use_current_stream()
    assert lib.take(arm) == [("kp1_set_stream", "handle", "stream")]
    route.use_current_stream()                                        # the wrapper kernels run on the base handle's stream
    assert lib.take(route) == [("kp1_set_stream", "base_handle", "stream")]
    out = arm.current_observation()
    assert out.shape == (4, 64) and out.dtype == torch.float32
    assert lib.take(arm, out=out) == [("kp1_observe", "handle", "out")]
    arm.snapshot()
    arm.restore()
    assert lib.take(arm) == [("kp1_state_snapshot", "handle"), ("kp1_state_restore", "handle")]
    assert not hasattr(route, "snapshot") and not hasattr(route, "restore")


# ------------------------------------------------------------------------------------------------------------------------ rng state
@pytest.mark.parametrize("family", ["arm", "route", "arm_pop", "route_pop"])
def test_rng_state_round_trip(lib, family):
    env = {"arm": lambda: _arm(lib, n=5), "route": lambda: _route(lib, n=5), "arm_pop": lambda: _arm_pop(lib, seeds=(1, 2, 3, 4, 5), n_per=1),
           "route_pop": lambda: _route_pop(lib, seeds=(1, 2, 3, 4, 5), n_per=1)}[family]()[0]
    lib.take()
    route = family.startswith("route")
    get, put, salt = ("kp1_route_rng_get", "kp1_route_rng_set", 2) if route else ("kp1_rng_get", "kp1_rng_set", 1)
    words = env.rng_state()
    assert lib.take(env) == [(get, "handle", "out")]
    assert words.dtype == np.uint64 and words.shape == (5, 6) and np.array_equal(words, rng_words(5, salt)) and int(words[0, 0]) > 2**63
    env.set_rng_state(words)
    assert lib.take(env) == [(put, "handle", tuple(tuple(int(v) for v in row) for row in rng_words(5, salt)))]
    if route:                                                         # the base env's streams are the base handle's own
        assert np.array_equal(env.base.rng_state(), rng_words(5, 1))
        assert lib.take(env) == [("kp1_rng_get", "base_handle", "out")]


# ------------------------------------------------------------------------------------------------------------------------ state and setters
def test_get_state_and_set_state(lib):
    env, _ = _arm(lib, n=3)
    route, _, _ = _route(lib, n=3)
    lib.take()
    for e, handle in ((env, "handle"), (route, "base_handle")):
        state = e.get_state()
        assert lib.take(e) == [("kp1_get_state", handle, "out", "out", "out", "out", "out")]
        assert list(state) == [k for k, _ in STATE_KEYS] and all(np.array_equal(state[k], state_values(3)[k]) for k in state)
    rng = np.random.default_rng(2)
    q, goal_q, pose = rng.normal(size=(3, 7)), rng.normal(size=7), rng.normal(size=(3, 6))
    env.set_state(q=q, goal_q=goal_q.astype(np.float32), goal_pose6=pose.tolist())
    assert lib.take(env) == [("kp1_set_state", "handle", tuple(map(tuple, q.tolist())), None, None, _full(goal_q.astype(np.float32), 3),
                              tuple(map(tuple, pose.tolist())), 1)]
    env.set_state(dq=q, prev_action=goal_q, capture_entry_metrics=False)
    assert lib.take(env) == [("kp1_set_state", "handle", None, tuple(map(tuple, q.tolist())), _full(goal_q, 3), None, None, 0)]
    env.set_state()
    assert lib.take(env) == [("kp1_set_state", "handle", None, None, None, None, None, 1)]
    with pytest.raises(ValueError):
        env.set_state(q=np.zeros((2, 7)))
    assert lib.take() == [] and env.launch_args_version == 0


def test_arm_setters_and_version_bumps(lib):
    dock = load_golden_config("dock_workspace_handoff_noop_ft_12env_raw")
    dock.handoff_states = dock.handoff_states[:2]
    env, _ = _arm(lib, n=2, cfg=dock)
    lib.take()
    version = 0

    def bumped(by: int) -> bool:
        nonlocal version
        version += by
        return env.launch_args_version == version

    env.set_curriculum_stage(4)
    assert lib.take(env) == [("kp1_set_stage", "handle", 4)] and bumped(1)
    assert env.get_curriculum_stage() == 3 and lib.take(env) == [("kp1_get_stage", "handle", "out")] and bumped(0)
    env.set_policy_mode("approach")
    assert lib.take(env) == [("kp1_set_mode", "handle", 0)] and env._mode_name == "approach" and bumped(1)
    with pytest.raises(ValueError, match="Unsupported policy mode 'bridge'"):
        env.set_policy_mode("bridge")
    assert lib.take() == [] and bumped(0)
    env.apply_dock_training_stage({"action_delta_scale": 0.5, "dock_reset": {"goal_noise": [0.25] * NJ}})
    assert dock.c.env.action_delta_scale == 0.5 and list(dock.c.dock_reset.goal_noise) == [0.25] * NJ
    assert lib.take(env) == [("kp1_update_config", "handle", cfg_item(dock.c))] and bumped(1)
    with pytest.raises(NotImplementedError, match="handoff buffer filter"):
        env.apply_dock_training_stage({"dock_reset": {"handoff_state_max_position_error_m": 1.0}})
    with pytest.raises(TypeError, match="unexpected keyword argument 'nope'"):
        env.apply_dock_training_stage({"dock_reset": {"nope": 1.0}})
    assert lib.take() == [] and bumped(0)
    states = dock.handoff_states[::-1]
    env.set_handoff_states(states)
    assert dock.handoff_states == states and dock.handoff_states is not states
    assert lib.take(env) == [("kp1_set_handoff_states", "handle", bytes(dock.handoff_array()), 2)] and bumped(1)
    env.set_handoff_states([])
    assert lib.take(env) == [("kp1_set_handoff_states", "handle", bytes(kcfg.HandoffState()), 0)] and bumped(1)
    env.set_obs_stride(64)
    assert lib.take(env) == [("kp1_set_obs_stride", "handle", 64)] and bumped(1)
    env.enable_reward_components()
    assert lib.take(env) == [("kp1_enable_reward_components", "handle", 1)] and env._reward_components_on is True and bumped(1)
    env.enable_reward_components(False)
    assert lib.take(env) == [("kp1_enable_reward_components", "handle", 0)] and env._reward_components_on is False and bumped(1)
    env.seed(3, 4)
    assert lib.take(env) == [("kp1_seed", "handle", 3, 4)] and bumped(0)
    env.set_route_stride_reset(None)
    assert len(lib.take(env)) == 1 and bumped(0)
    assert env.env_method("set_curriculum_stage", 2) == [None, None] and lib.take(env) == [("kp1_set_stage", "handle", 2)] and bumped(1)
    assert env.env_method("get_curriculum_stage") == [3, 3] and bumped(0)

    approach, _ = _arm(lib, n=2)
    lib.take()
    approach.apply_dock_training_stage({"action_delta_scale": 0.5})   # arm_kinematic_env.py:459: not a dock env, nothing happens
    assert lib.take() == [] and approach.launch_args_version == 0


def test_arm_info_and_reward_components(lib):
    for real, ts in (("f32", "<f4"), ("f64", "<f8")):
        env, _ = _arm(lib, n=3, real=real)
        lib.take()
        info = env.info()
        assert lib.take(env) == [("kp1_get_info", "handle", "out")]
        fields = [name for name, _ in kcfg.InfoView._fields_]
        ptr = {name: 0x100000 + 0x100 * j for j, name in enumerate(fields)}
        reals = {"position_error_norm": (3,), "orientation_error_norm": (3,), "min_position_error": (3,), "executed_delta_q_l2": (3,), "action_l2": (3,),
                 "delta_q_change_l2": (3,), "q": (7, 3), "dq": (7, 3), "prev_action": (7, 3), "goal_q": (7, 3), "goal_pose6": (6, 3), "ee_pose6": (6, 3),
                 "entry_metrics": (4, 3)}
        ints = {"step_count": "episode_step", "dwell_count": "dwell_count", "near_goal_entry_count": "near_goal_entry_count",
                "near_goal_drift_count": "near_goal_drift_count", "flags": "flags", "stage_index": "stage_index"}
        want = {k: ("view", ptr[k], shape, ts, CPU) for k, shape in reals.items()}
        want.update({k: ("view", ptr[f], (3,), "<i4", CPU) for k, f in ints.items()})
        assert info == want and list(info) == list(want)
        names, comps = env.reward_components()
        assert names == ["component_0_0", "component_0_1"] and comps == ("view", 0x7700, (5, 3), ts, CPU)
        assert lib.take(env) == [("kp1_get_reward_components", "handle", "out", "out"), ("kp1_num_components", 0), ("kp1_component_name", 0, 0),
                                 ("kp1_component_name", 0, 1)]
        env.reset(options={"policy_mode": "dock"})                    # the names follow the mode of the last reset
        lib.take()
        assert env.reward_components()[0] == ["component_1_0", "component_1_1"]
    obs = torch.arange(2 * 56, dtype=torch.float32).reshape(2, 56)
    split = ve.ArmKinematicVecEnv.obs_dict(obs)
    assert list(split) == list(kcfg.OBS_LAYOUT) and all(torch.equal(split[k], obs[:, s:s + n]) for k, (s, n) in kcfg.OBS_LAYOUT.items())


def test_route_setters_info_and_env_method(lib, monkeypatch):
    env, _, route_cfg = _route(lib, n=3, real="f64")
    lib.take()
    env.set_route_window(max_route_index=77, min_route_index=5)
    assert lib.take(env) == [("kp1_route_set_window", "handle", 5, 77)]
    assert (route_cfg.reset.min_route_index, route_cfg.reset.max_route_index) == (5, 77)
    env.set_route_window(max_route_index=9)
    assert lib.take(env) == [("kp1_route_set_window", "handle", 1, 9)] and route_cfg.reset.min_route_index == 1
    assert env.env_method("set_route_window", max_route_index=12, min_route_index=2) == [None] * 3     # SB3's env_method, with keywords
    assert lib.take(env) == [("kp1_route_set_window", "handle", 2, 12)]
    assert env.env_method("seed", 4, 1) == [None] * 3 and lib.take(env) == [("kp1_route_seed", "handle", 4, 1)]
    assert env.launch_args_version == 0
    env.enable_reward_components()
    env.enable_reward_components(False)
    assert lib.take(env) == [("kp1_route_enable_reward_components", "handle", 1), ("kp1_route_enable_reward_components", "handle", 0)]
    assert env._reward_components_on is False and env.launch_args_version == 2 and env.base.launch_args_version == 0
    names, comps = env.reward_components()
    assert names == list(rcfg.COMPONENT_NAMES) and comps == ("view", 0x7800, (len(rcfg.COMPONENT_NAMES), 3), "<f8", CPU)
    assert lib.take(env) == [("kp1_route_get_reward_components", "handle", "out")]

    fields = [name for name, _ in re_._RouteInfoView._fields_]
    ptr = {name: 0x100000 + 0x100 * j for j, name in enumerate(fields)}
    flags = env.episode_flags
    monkeypatch.setattr(torch, "stack", lambda views: ("stacked", tuple(views)))
    want_flags = ("stacked", tuple(("view", ptr[f], (3,), "|u1", CPU) for f in ("route_ready", "orientation_hit", "route_regression")))
    assert flags() == want_flags and lib.take(env) == [("kp1_route_get_info", "handle", "out")]
    assert flags() == want_flags and lib.take(env) == []             # the views are taken once

    class _Index:                                                     # stands for the route_index view: info() reads it back to pick host rows
        def long(self): return self
        def clamp(self, lo, hi): return self
        def cpu(self): return self
        def numpy(self): return np.array([0, 2, env.n_waypoints - 1])

    monkeypatch.setattr(re_, "_view", lambda p, shape, ts, dev: _Index() if p == ptr["route_index"] else ("view", p, tuple(shape), ts, dev))
    info = env.info()
    assert lib.take(env) == [("kp1_route_get_info", "handle", "out"), ("kp1_get_info", "base_handle", "out")]
    assert info["q"] == ("view", 0x100000 + 0x100 * 6, (7, 3), "<f8", CPU)                       # the base env's keys
    ints = {"start_route_index": "start_route_index", "last_route_index": "last_route_index", "route_reset_mode": "reset_mode",
            "route_ready_streak": "ready_streak", "route_completed_waypoints": "completed_waypoints"}
    bools = {"route_ready": "route_ready", "route_waypoint_success": "waypoint_success", "route_regression": "route_regression",
             "route_orientation_hit": "orientation_hit"}
    assert all(info[k] == ("view", ptr[f], (3,), "<i4", CPU) for k, f in ints.items())
    assert all(info[k] == ("view", ptr[f], (3,), "|u1", CPU) for k, f in bools.items())
    assert info["route_q_error_norm"] == ("view", ptr["q_error_norm"], (3,), "<f8", CPU)
    assert info["nearest_route_q_distance"] == ("view", ptr["nearest_route_q_distance"], (3,), "<f8", CPU)
    rows = [0, 2, env.n_waypoints - 1]
    assert np.array_equal(info["route_progress_m"].numpy(), env.route_progress_m[rows]) and np.array_equal(info["route_chunk_id"].numpy(), env.chunk_id[rows])
    assert len(info) == len(kcfg.InfoView._fields_) - 2 + 14

    for width, layout in ((80, rcfg.ROUTE_OBS_LAYOUT), (128, rcfg.ROUTE_OBS_LAYOUT), (56, kcfg.OBS_LAYOUT), (64, kcfg.OBS_LAYOUT)):
        obs = torch.arange(2 * width, dtype=torch.float32).reshape(2, width)
        split = re_.RouteVecEnv.obs_dict(obs)
        assert list(split) == list(layout) and all(torch.equal(split[k], obs[:, o:o + w]) for k, (o, w) in layout.items())


def test_route_population_windows(lib):
    pop, _, route_cfg = _route_pop(lib, seeds=(1, 2, 3), n_per=2)
    lib.take()
    first = (int(route_cfg.reset.min_route_index), int(route_cfg.reset.max_route_index))
    pop.set_replica_window(1, max_route_index=60, min_route_index=3)
    assert lib.take(pop) == [("kp1_route_set_replica_window", "handle", 1, 3, 60)]
    assert [pop.window(k) for k in range(3)] == [first, (3, 60), first]
    assert (int(route_cfg.reset.min_route_index), int(route_cfg.reset.max_route_index)) == first    # the shared config keeps the first window
    pop.set_replica_window(2, max_route_index=20)
    assert lib.take(pop) == [("kp1_route_set_replica_window", "handle", 2, 1, 20)] and pop.window(2) == (1, 20)
    pop.set_route_window(max_route_index=80, min_route_index=2)
    assert lib.take(pop) == [("kp1_route_set_window", "handle", 2, 80)]
    assert [pop.window(k) for k in range(3)] == [(2, 80)] * 3 and (route_cfg.reset.min_route_index, route_cfg.reset.max_route_index) == (2, 80)
    assert pop.launch_args_version == 0


def test_close_destroys_once(lib):
    arm, _ = _arm(lib, n=2)
    route, _, _ = _route(lib, n=2)
    lib.take()
    arm.close()
    arm.close()
    assert lib.take(handle=0xA100) == [("kp1_destroy", "handle")] and not arm._handle.value
    base = route.base
    route.close()
    route.close()
    assert lib.take(base_handle=0xA200, handle=0xA300) == [("kp1_route_destroy", "handle"), ("kp1_destroy", "base_handle")]
    assert not route._handle.value and not base._handle.value
    for cls in (ve.ArmKinematicVecEnv, ve.ArmKinematicPopulationVecEnv, re_.RouteVecEnv, re_.RoutePopulationVecEnv):
        cls.__new__(cls).__del__()                                    # an instance whose constructor refused owns nothing
    assert lib.take() == []


# ------------------------------------------------------------------------------------------------------------------------ populations
def test_population_refusals(lib):
    pop, cfg = _arm_pop(lib)
    rpop, _, _ = _route_pop(lib)
    lib.take()
    for bad in (lambda: pop.seed(3), lambda: pop.reset(seed=3), lambda: rpop.seed(3, 1), lambda: rpop.reset(seed=3)):
        with pytest.raises(ValueError, match=r"a population (route )?env keeps the per-block seeds it was created with \(env i of replica k: seeds\[k\] \+ i\)"):
            bad()
    for bad in (lambda: pop.set_policy_mode("dock"), lambda: pop.reset(options={"policy_mode": "dock"})):
        with pytest.raises(ValueError, match=r"a population env runs its config's mode \(approach\) only"):
            bad()
    assert lib.take() == []
    pop.set_policy_mode("approach")
    pop.reset(options={"policy_mode": "approach"})
    assert [c[0] for c in lib.take(pop)] == ["kp1_set_mode", "kp1_reset"] and pop.launch_args_version == 1
    pop.dock_population = object()
    with pytest.raises(ValueError, match="a DockReverseCurriculumPopulation is attached"):
        pop.apply_dock_training_stage({})
    for k in (-1, 2):
        with pytest.raises(IndexError, match=f"replica {k} of a population of 2"):
            pop.replica(k)
    for k in (-1, 3):                # the one accepted change of DESIGN.md section 45: before it, the view was built and failed on seeds[k] or in C
        with pytest.raises(IndexError, match=f"replica {k} of a population of 3"):
            rpop.replica(k)
    assert lib.take() == []
    assert issubclass(ve.ArmKinematicPopulationVecEnv, ve.ArmKinematicVecEnv) and issubclass(re_.RoutePopulationVecEnv, re_.RouteVecEnv)
    assert ve.MAX_REPLICAS == 16


@pytest.mark.parametrize("family", ["arm", "route"])
def test_replica_views(lib, family):
    pop = (_arm_pop(lib, seeds=(11, 12, 13), n_per=2) if family == "arm" else _route_pop(lib, seeds=(11, 12, 13), n_per=2))[0]
    lib.take()
    view = pop.replica(1)
    assert type(view) is (ve.ArmKinematicReplicaEnv if family == "arm" else re_.RouteReplicaEnv)
    # what PPO's setup, ReplicaView, checkpoint.save and evaluate.py read
    assert view.pop is pop and view.k == 1 and view.seed == 12 and view.n_envs == 2
    assert view.device == CPU and view.dtype == torch.float32 and view.config is pop.config
    assert view.obs_dim == (56 if family == "arm" else 80) and view.obs_stride == pop.obs_stride and view.launch_args_version == 0
    assert not hasattr(view, "is_population") and not hasattr(view, "_reward_components_on") and not hasattr(view, "step_into")
    assert hasattr(view, "snapshot") == hasattr(view, "restore") == (family == "arm")           # PPO._capture_rollout decides by this
    assert hasattr(view, "route_cfg") == hasattr(view, "n_waypoints") == hasattr(view, "route_q") == hasattr(view, "route_progress_m") == (family == "route")
    set_stride = "kp1_set_obs_stride" if family == "arm" else "kp1_route_set_obs_stride"
    view.set_obs_stride(pop.obs_stride)                                # forwarded only on a change
    assert lib.take(pop) == []
    view.set_obs_stride(128)
    assert lib.take(pop) == [(set_stride, "handle", 128)] and view.obs_stride == pop.obs_stride == 128 and pop.obs.shape == (6, 128)
    assert view.launch_args_version == pop.launch_args_version == (1 if family == "arm" else 0)
    pop.replica(2).set_obs_stride(128)
    assert lib.take(pop) == []
    view.use_current_stream()
    assert lib.take(pop) == [("kp1_set_stream", "handle" if family == "arm" else "base_handle", "stream")]
    with pytest.raises(TypeError, match=rf"a replica of an? {type(pop).__name__} is reset through the population handle \(one reset of all replicas\)"):
        view.reset(seed=3)
    assert view.close() is None and lib.take() == [] and pop._handle.value
    if family == "arm":
        view.snapshot()
        view.restore()
        assert lib.take(pop) == [("kp1_state_snapshot", "handle"), ("kp1_state_restore", "handle")]
    else:
        assert view.route_q is pop.route_q and view.n_waypoints == pop.n_waypoints and view.route_progress_m is pop.route_progress_m
        shared = bytes(pop.route_cfg)
        pop.set_replica_window(1, max_route_index=66, min_route_index=4)
        cfg = view.route_cfg
        assert type(cfg) is rcfg.RouteConfig and cfg is not pop.route_cfg and (cfg.reset.min_route_index, cfg.reset.max_route_index) == (4, 66)
        assert bytes(pop.route_cfg) == shared                         # a copy: the population's config is untouched
        other = pop.replica(0).route_cfg
        assert bytes(other) == shared and other is not pop.route_cfg
        cfg.reset.max_route_index = 5
        assert bytes(pop.route_cfg) == shared and view.route_cfg.reset.max_route_index == 66


# ------------------------------------------------------------------------------------------------------------------------ route chain
def test_route_chain_calls(lib):
    env, _, _ = _route(lib, n=3)
    lib.take()
    chain = env.chain(2, [5, 6, 7], stop_on_failure=True)
    assert lib.take(env, chain=0xC000) == [("kp1_route_chain_create", "handle", (2, 2, 2), (5, 6, 7), 3, 1, "out"), ("kp1_route_chain_get_view", "chain", "out")]
    assert chain.max_len == 4 and chain._records == ("view", 0x200000, (3 * 4 * 312,), "|u1", CPU)
    assert chain._n_records == ("view", 0x200100, (3,), "<i4", CPU) and chain._n_alive == ("view", 0x200200, (1,), "<i4", CPU)
    b = _caller_buffers(3, 128)
    tags = torch.zeros(3, 2, dtype=torch.int32)
    mlp = types.SimpleNamespace(_h=C.c_void_p(0xD000), _stream=lambda: C.c_void_p(STREAM))
    names = dict(b, tags=tags, chain=0xC000, mlp=0xD000)
    chain.begin(b["c_obs"])
    chain.step(b["c_act"], b["c_obs"], b["c_rew"], b["c_done"])
    chain.step(b["c_act"], b["c_obs"], b["c_rew"], b["c_done"], tags)
    assert lib.take(env, **names) == [("kp1_route_chain_begin", "handle", "chain", "c_obs"),
                                      ("kp1_route_chain_step", "handle", "chain", "c_act", "c_obs", "c_rew", "c_done", None),
                                      ("kp1_route_chain_step", "handle", "chain", "c_act", "c_obs", "c_rew", "c_done", "tags")]
    chain.forward_step(mlp, b["c_obs"], b["c_term"], b["c_rew"], b["c_done"])
    chain.forward_step(mlp, b["c_obs"], b["c_obs"], b["c_rew"], b["c_done"], action=b["c_act"], tags=tags)
    chain.run(mlp, b["c_obs"], b["c_rew"], b["c_done"], 9)
    chain.close()
    chain.close()
    assert lib.take(env, **names) == [
        ("kp1_mlp_forward_route_chain_step", "mlp", "handle", "chain", "c_obs", 128, None, "c_term", "c_rew", "c_done", None, "stream"),
        ("kp1_mlp_forward_route_chain_step", "mlp", "handle", "chain", "c_obs", 128, "c_act", "c_obs", "c_rew", "c_done", "tags", "stream"),
        ("kp1_route_chain_run", "mlp", "handle", "chain", "c_obs", 128, "c_rew", "c_done", 9, "stream"),
        ("kp1_route_chain_destroy", "handle", "chain")]


# ------------------------------------------------------------------------------------------------------------------------ free functions
def test_fk_pose6_refusals_in_their_order(lib):
    class _OnDevice:
        """a (n, 7) tensor of a dtype no kernel takes that says it is on the device"""
        ndim, shape, is_cuda, dtype, device = 2, (3, 7), True, torch.int32, CPU

        def contiguous(self):
            return self

    for bad in (torch.zeros(7), torch.zeros(3, 6), torch.zeros(3, 6, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"Expected q of shape \(n, 7\)"):
            ve.fk_pose6(bad)
    for dtype in (torch.float32, torch.int32):                        # the device is asked for before the dtype
        with pytest.raises(native.Kp1Error, match="fk_pose6 needs a device tensor; there is no CPU fallback"):
            ve.fk_pose6(torch.zeros(3, 7, dtype=dtype))
    with pytest.raises(ValueError, match="float32 or float64"):
        ve.fk_pose6(_OnDevice())
    assert lib.take() == []
