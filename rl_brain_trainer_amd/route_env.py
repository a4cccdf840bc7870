"""Route-curriculum environments on the device: N ``RouteKinematicEnv`` / ``RouteSequenceKinematicEnv`` at once.

Mirror of kinematic_phase1/route/route_env.py:29-212 and route_sequence_env.py:29-278 (which of the two is chosen by
``route.sequence.enabled``, like train_route_curriculum.py:104-107) behind the C ABI of include/kp1_route.h.  Same reset
options (``route_index``, ``start_route_index``, ``initial_q`` / ``initial_dq`` / ``initial_prev_action`` for the sequence
env), same ``set_route_window``, same info keys; observations are rows of 56 floats, or 80 with ``include_route_keys`` (the
17 Dict keys in SB3's sorted order: route_config.ROUTE_OBS_LAYOUT).  Env i owns ``default_rng(seed + first_env_id + i)`` for
the wrapper's reset stream, as ``make_vec_env(make_env, n_envs, seed)`` gives it.
"""
from __future__ import annotations

import ctypes as C
from typing import Any

import numpy as np
import torch

from . import config as kcfg
from . import native
from . import route_config as rcfg
from .vec_env import ArmKinematicVecEnv, DeviceEnvHandle, PopulationEnvHandle, ReplicaEnv, _view


class _RouteResetOpts(C.Structure):
    _fields_ = [("route_index", C.c_void_p), ("start_route_index", C.c_void_p), ("initial_q", C.c_void_p), ("initial_dq", C.c_void_p),
                ("initial_prev_action", C.c_void_p), ("evaluator_state", C.c_int32), ("pad_", C.c_int32)]


class _RouteInfoView(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("route_index", "start_route_index", "last_route_index", "reset_mode", "ready_streak", "completed_waypoints",
                                          "route_ready", "waypoint_success", "route_regression", "orientation_hit", "q_error_norm",
                                          "nearest_route_q_distance")]


# include/kp1_route.h kp1_route_chain_record
CHAIN_RECORD = np.dtype([(n, "<i4") for n in ("route_index", "success", "route_ready_hit", "max_ready_streak", "first_ready_step", "steps")] +
                        [(n, "<f8") for n in ("final_position_error", "final_orientation_error", "final_q_error", "min_position_error",
                                              "min_orientation_error", "min_q_error", "final_action_magnitude", "final_dq_norm")] +
                        [(n, "<f8", (kcfg.NJ,)) for n in ("final_q", "final_dq", "final_prev_action", "start_q")])
assert CHAIN_RECORD.itemsize == 312


class RouteVecEnv(DeviceEnvHandle):
    """``route_q``: [W, 7] joint goals of the dense route (route_config.load_route_q); ``base_config``: the env block of the route
    YAML (approach mode); ``route_cfg``: route_config.route_config_from_dict(cfg, max_route_index=first prefix)."""

    def __init__(self, base_config: kcfg.EnvConfig, route_cfg: rcfg.RouteConfig, route_q: np.ndarray, n_envs: int, *, device: int | torch.device = 0,
                 seed: int = 0, first_env_id: int = 0, real: str = "f32", reward_components: bool = False) -> None:
        self.base = ArmKinematicVecEnv(base_config, n_envs, device=device, seed=seed, first_env_id=first_env_id, real=real)
        self.L = self.base.L
        self.config = base_config
        self.route_cfg = route_cfg
        self.n_envs = int(n_envs)
        self.device = self.base.device
        self.dtype = self.base.dtype
        self.route_q = np.ascontiguousarray(route_q, dtype=np.float64)
        if self.route_q.ndim != 2 or self.route_q.shape[1] != kcfg.NJ:
            raise ValueError("route_q must have shape (n_waypoints, 7)")
        self.n_waypoints = int(self.route_q.shape[0])
        self._handle = C.c_void_p()
        with torch.cuda.device(self.device):
            self._create(route_cfg, seed, first_env_id)
        self.obs_dim = int(self.L.kp1_route_obs_dim(self._handle))
        self._alloc_buffers(self.obs_dim)
        W = self.n_waypoints
        self.poses6 = np.zeros((W, 6))
        self.route_progress_m = np.zeros(W)
        self.next_q_delta = np.zeros((W, kcfg.NJ))
        self.chunk_id = np.zeros(W, dtype=np.int32)
        native.check(self.L.kp1_route_get_dataset(self._handle, C.c_void_p(self.poses6.ctypes.data), C.c_void_p(self.route_progress_m.ctypes.data),
                                                  C.c_void_p(self.next_q_delta.ctypes.data), C.c_void_p(self.chunk_id.ctypes.data)))
        self._keep: list[Any] = []
        self._reward_components_on = False
        self.launch_args_version = 0     # bumped by setters that change which kernels a step launches (PPO re-captures its rollout graph)
        if reward_components:
            self.enable_reward_components(True)

    def _create(self, route_cfg: rcfg.RouteConfig, seed: int, first_env_id: int) -> None:
        native.check(self.L.kp1_route_create(self.base._handle, C.byref(route_cfg), C.c_void_p(self.route_q.ctypes.data), self.n_waypoints, int(seed),
                                             int(first_env_id), C.byref(self._handle)))

    # ------------------------------------------------------------------ the family's C calls behind DeviceEnvHandle
    def _step_call(self, *ptrs: Any) -> int:
        return self.L.kp1_route_step(self._handle, *ptrs)

    def _rng_get_call(self, arr: Any) -> int:
        return self.L.kp1_route_rng_get(self._handle, arr)

    def _rng_set_call(self, arr: Any) -> int:
        return self.L.kp1_route_rng_set(self._handle, arr)

    def _set_obs_stride_call(self, stride: int) -> int:
        return self.L.kp1_route_set_obs_stride(self._handle, stride)      # (unlike the arm handle's, no launch_args_version bump)

    def _destroy(self) -> None:
        self.L.kp1_route_destroy(self._handle)

    def close(self) -> None:
        """the wrapper first, then the base handle it was made on"""
        super().close()
        self.base.close()

    # ------------------------------------------------------------------ reference API
    def set_route_window(self, *, max_route_index: int, min_route_index: int = 1) -> None:
        native.check(self.L.kp1_route_set_window(self._handle, int(min_route_index), int(max_route_index)))
        self.route_cfg.reset.min_route_index = int(min_route_index)
        self.route_cfg.reset.max_route_index = int(max_route_index)

    def seed(self, seed: int, first_env_id: int = 0) -> None:
        native.check(self.L.kp1_route_seed(self._handle, int(seed), int(first_env_id)))

    def reset(self, *, seed: int | None = None, options: dict[str, Any] | None = None, mask: torch.Tensor | None = None) -> torch.Tensor:
        """options: {"route_index": int | [N], "start_route_index", "initial_q" [N,7], "initial_dq", "initial_prev_action"} or None = sample.
        ``evaluator_state=True`` makes the single-waypoint env honour the initial state too (the sequential evaluator's chained resets)."""
        if seed is not None:
            self.seed(seed)
        opts = None
        self._keep = []
        if options and "route_index" in options:
            n = self.n_envs

            def ints(v):
                t = torch.as_tensor(np.broadcast_to(np.asarray(v, dtype=np.int32), (n,)).copy(), device=self.device)
                self._keep.append(t)
                return t.data_ptr()

            def mats(v):
                t = torch.as_tensor(np.broadcast_to(np.asarray(v, dtype=np.float64), (n, kcfg.NJ)).copy(), device=self.device)
                self._keep.append(t)
                return t.data_ptr()

            opts = _RouteResetOpts()
            opts.route_index = ints(options["route_index"])
            opts.start_route_index = ints(options["start_route_index"]) if "start_route_index" in options else None
            for key in ("initial_q", "initial_dq", "initial_prev_action"):
                setattr(opts, key, mats(options[key]) if key in options else None)
            opts.evaluator_state = int(bool(options.get("evaluator_state", False)))
        m = self._reset_mask(mask)
        if m is not None:
            self._keep.append(m)
        native.check(self.L.kp1_route_reset(self._handle, native.ptr(m), C.byref(opts) if opts is not None else None, native.ptr(self.obs)))
        return self.obs

    def use_current_stream(self) -> None:
        """Order this handle's launches on torch's current stream (the wrapper kernels run on the base handle's stream)."""
        self.base.use_current_stream()

    @staticmethod
    def obs_dict(obs: torch.Tensor) -> dict[str, torch.Tensor]:
        layout = rcfg.ROUTE_OBS_LAYOUT if obs.shape[-1] in (rcfg.ROUTE_OBS_DIM, 128) else kcfg.OBS_LAYOUT   # 128 / 64: padded PPO rows
        return {k: obs[..., o:o + w] for k, (o, w) in layout.items()}

    def info(self) -> dict[str, torch.Tensor]:
        """Base env info (ArmKinematicVecEnv.info) plus the wrapper's keys; tensors are views of device state."""
        v = _RouteInfoView()
        native.check(self.L.kp1_route_get_info(self._handle, C.byref(v)))
        n, ts = self.n_envs, self._typestr
        out = dict(self.base.info())
        for key, name in (("route_index", "route_index"), ("start_route_index", "start_route_index"), ("last_route_index", "last_route_index"),
                          ("route_reset_mode", "reset_mode"), ("route_ready_streak", "ready_streak"), ("route_completed_waypoints", "completed_waypoints")):
            out[key] = _view(getattr(v, name), (n,), "<i4", self.device)
        for key, name in (("route_ready", "route_ready"), ("route_waypoint_success", "waypoint_success"), ("route_regression", "route_regression"),
                          ("route_orientation_hit", "orientation_hit")):
            out[key] = _view(getattr(v, name), (n,), "|u1", self.device)
        out["route_q_error_norm"] = _view(v.q_error_norm, (n,), ts, self.device)
        out["nearest_route_q_distance"] = _view(v.nearest_route_q_distance, (n,), ts, self.device)
        idx = out["route_index"].long().clamp(0, self.n_waypoints - 1).cpu().numpy()
        out["route_progress_m"] = torch.as_tensor(self.route_progress_m[idx])
        out["route_chunk_id"] = torch.as_tensor(self.chunk_id[idx])
        return out

    def episode_flags(self) -> torch.Tensor:
        """[3, N] uint8 device tensor (route_ready, route_orientation_hit, route_regression) of the last step: what the prefix curriculum
        reads per finished episode, without building the whole info dict."""
        if getattr(self, "_flag_views", None) is None:
            v = _RouteInfoView()
            native.check(self.L.kp1_route_get_info(self._handle, C.byref(v)))
            self._flag_views = tuple(_view(getattr(v, name), (self.n_envs,), "|u1", self.device) for name in ("route_ready", "orientation_hit", "route_regression"))
        return torch.stack(self._flag_views)

    def enable_reward_components(self, enable: bool = True) -> None:
        native.check(self.L.kp1_route_enable_reward_components(self._handle, int(enable)))
        self._reward_components_on = bool(enable)     # the one-launch rollout step does not record them: the trainers fall back
        self.launch_args_version += 1

    def reward_components(self) -> tuple[list[str], torch.Tensor]:
        p = C.c_void_p()
        native.check(self.L.kp1_route_get_reward_components(self._handle, C.byref(p)))
        return list(rcfg.COMPONENT_NAMES), _view(p.value, (len(rcfg.COMPONENT_NAMES), self.n_envs), self._typestr, self.device)

    def get_state(self) -> dict[str, np.ndarray]:
        return self.base.get_state()

    def chain(self, start_index, end_index, *, stop_on_failure: bool = False) -> "RouteChain":
        """a chained sequential evaluation over every env of this handle (RouteChain); indices are ints or one per env"""
        return RouteChain(self, start_index, end_index, stop_on_failure=stop_on_failure)


class RouteChain:
    """Chain state of a route handle (include/kp1_route.h, kp1_route_chain_*): row r runs the sequential evaluation of the waypoints
    ``start_index[r] .. end_index[r]``, each episode starting from the previous one's final (q, dq, prev_action).  ``begin`` resets every row to
    its first waypoint; ``step`` is one route step of all rows plus kp1_route_chain_kernel (bookkeeping, records, hand-over), with no host read.
    ``forward_step`` is the policy forward and ``step`` in ONE launch and ``run`` a span of such lock steps in one launch (hidden 64 / 128;
    neither steps a row whose chain has ended).  ``alive()`` reads the device counter of running rows; ``records()`` the finished waypoints
    of every row."""

    def __init__(self, env: RouteVecEnv, start_index, end_index, *, stop_on_failure: bool = False) -> None:
        n = env.n_envs
        self.env = env
        self.start = np.ascontiguousarray(np.broadcast_to(np.asarray(start_index, dtype=np.int32), (n,)))
        self.end = np.ascontiguousarray(np.broadcast_to(np.asarray(end_index, dtype=np.int32), (n,)))
        self.stop_on_failure = bool(stop_on_failure)
        self._h = C.c_void_p()
        with torch.cuda.device(env.device):
            native.check(env.L.kp1_route_chain_create(env._handle, C.c_void_p(self.start.ctypes.data), C.c_void_p(self.end.ctypes.data), n,
                                                      int(self.stop_on_failure), C.byref(self._h)))
        v = native.RouteChainView()
        native.check(env.L.kp1_route_chain_get_view(self._h, C.byref(v)))
        self.max_len = int(v.max_len)
        self._records = _view(v.records, (n * self.max_len * CHAIN_RECORD.itemsize,), "|u1", env.device)
        self._n_records = _view(v.n_records, (n,), "<i4", env.device)
        self._n_alive = _view(v.n_alive, (1,), "<i4", env.device)

    def begin(self, obs: torch.Tensor) -> None:
        native.check(self.env.L.kp1_route_chain_begin(self.env._handle, self._h, native.ptr(obs)))

    def step(self, actions: torch.Tensor, obs: torch.Tensor, reward: torch.Tensor, done: torch.Tensor, tags: torch.Tensor | None = None) -> None:
        """actions [R, 7] f32 (read), obs [R, stride] (next observations), reward [R], done [R] uint8, tags [R, 2] int32 or None"""
        p = native.ptr
        native.check(self.env.L.kp1_route_chain_step(self.env._handle, self._h, p(actions), p(obs), p(reward), p(done), p(tags)))

    def forward_step(self, mlp, obs: torch.Tensor, next_obs: torch.Tensor, reward: torch.Tensor, done: torch.Tensor, *,
                     action: torch.Tensor | None = None, tags: torch.Tensor | None = None) -> None:
        """``mlp.forward(obs, clipped=action)`` + ``step(action, next_obs, reward, done, tags)`` in ONE launch (kp1_mlp_forward_route_chain_step),
        bit for bit for every row whose chain is alive.  ``mlp``: an mlp.MlpKernels handle at hidden 64 / 128 whose replicas own the rows
        replica-major; ``obs`` at the pitch set with ``env.set_obs_stride``; ``next_obs`` is ``obs`` itself (in place) or disjoint from it.  A
        row whose chain has ended is not stepped: it gets its {-1, -1} tag and nothing else of it is written."""
        assert obs.is_contiguous() and obs.dtype == torch.float32 and obs.shape[0] == self.env.n_envs
        p = native.ptr
        native.check(self.env.L.kp1_mlp_forward_route_chain_step(mlp._h, self.env._handle, self._h, p(obs), int(obs.shape[1]), p(action), p(next_obs),
                                                                 p(reward), p(done), p(tags), mlp._stream()))

    def run(self, mlp, obs: torch.Tensor, reward: torch.Tensor, done: torch.Tensor, n_steps: int) -> None:
        """``n_steps`` lock steps (1 .. native.ROUTE_CHAIN_RUN_MAX_STEPS) of ``forward_step`` in ONE launch, in place on ``obs``
        (kp1_route_chain_run); ``alive()`` afterwards is the number of rows still running after the last step."""
        assert obs.is_contiguous() and obs.dtype == torch.float32 and obs.shape[0] == self.env.n_envs
        native.check(self.env.L.kp1_route_chain_run(mlp._h, self.env._handle, self._h, native.ptr(obs), int(obs.shape[1]), native.ptr(reward),
                                                    native.ptr(done), int(n_steps), mlp._stream()))

    def alive(self) -> int:
        """rows still running after the last step (synchronises)"""
        return int(self._n_alive.item())

    def records(self) -> list[np.ndarray]:
        """per row, the CHAIN_RECORD array of its finished waypoints in route order (synchronises)"""
        counts = self._n_records.cpu().numpy()
        table = np.frombuffer(self._records.cpu().numpy().tobytes(), dtype=CHAIN_RECORD).reshape(self.env.n_envs, self.max_len)
        return [table[r, :int(counts[r])].copy() for r in range(self.env.n_envs)]

    def close(self) -> None:
        if self._h.value:
            self.env.L.kp1_route_chain_destroy(self.env._handle, self._h)
            self._h = C.c_void_p()


class RouteReplicaEnv(ReplicaEnv):
    """Replica k of a RoutePopulationVecEnv: with the route dataset the evaluators read, and the route config as this replica sees it.  (No
    ``snapshot`` / ``restore``: PPO rolls a graph warm-up on a route env back with a fresh reset.)"""

    def __init__(self, pop: "RoutePopulationVecEnv", k: int) -> None:
        super().__init__(pop, k)
        self.route_q, self.n_waypoints, self.route_progress_m = pop.route_q, pop.n_waypoints, pop.route_progress_m

    @property
    def route_cfg(self) -> rcfg.RouteConfig:
        """a copy of the shared config with replica k's reset window"""
        cfg = rcfg.RouteConfig.from_buffer_copy(self.pop.route_cfg)
        cfg.reset.min_route_index, cfg.reset.max_route_index = self.pop.window(self.k)
        return cfg


class RoutePopulationVecEnv(PopulationEnvHandle, RouteVecEnv):
    """K route envs of ``n_per_replica`` envs each in ONE handle (include/kp1_route.h, kp1_route_create_population): block k = rows
    [k N, (k + 1) N) is replica k, and is bit for bit ``RouteVecEnv(..., n_per_replica, seed=seeds[k])``.  One ``step_into`` / ``reset``
    covers all K N rows, so a population rollout is one route step per env step whatever K is -- the [K N, obs_w] buffers are the population
    rollout's replica-major layout.  The config is shared except the reset window, which each replica has of its own (``set_route_window``
    sets every window, ``set_replica_window`` one).  ``replica(k)`` is a view with what PPO's setup and ``checkpoint.save`` read."""

    replica_type = RouteReplicaEnv

    def __init__(self, base_config: kcfg.EnvConfig, route_cfg: rcfg.RouteConfig, route_q: np.ndarray, seeds: list[int], n_per_replica: int, *,
                 device: int | torch.device = 0, reward_components: bool = False) -> None:
        self._take_seeds(seeds)
        n_envs = self._take_blocks(n_per_replica)
        self._windows = [(int(route_cfg.reset.min_route_index), int(route_cfg.reset.max_route_index))] * self.K
        super().__init__(base_config, route_cfg, route_q, n_envs, device=device, seed=self.seeds[0], real="f32", reward_components=reward_components)

    def _create(self, route_cfg: rcfg.RouteConfig, seed: int, first_env_id: int) -> None:
        seeds = (C.c_uint64 * self.K)(*self.seeds)
        native.check(self.L.kp1_route_create_population(self.base._handle, C.byref(route_cfg), C.c_void_p(self.route_q.ctypes.data), self.n_waypoints,
                                                        C.cast(seeds, C.c_void_p), self.K, C.byref(self._handle)))

    def set_route_window(self, *, max_route_index: int, min_route_index: int = 1) -> None:
        super().set_route_window(max_route_index=max_route_index, min_route_index=min_route_index)
        self._windows = [(int(min_route_index), int(max_route_index))] * self.K

    def set_replica_window(self, k: int, *, max_route_index: int, min_route_index: int = 1) -> None:
        native.check(self.L.kp1_route_set_replica_window(self._handle, int(k), int(min_route_index), int(max_route_index)))
        self._windows[k] = (int(min_route_index), int(max_route_index))

    def window(self, k: int) -> tuple[int, int]:
        """host copy of replica k's reset window (a tracker promotion moves the device copy; RoutePrefixCurriculumPopulation.read(k) syncs it)"""
        return self._windows[k]
