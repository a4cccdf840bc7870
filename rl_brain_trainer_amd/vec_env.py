"""Batched MI355X environment behind the reference's env API.

``ArmKinematicVecEnv`` is N ``ArmKinematicEnv`` instances (reference:
kinematic_phase1/envs/arm_kinematic_env.py:69-560) living on one GPU, stepped by one HIP
kernel launch through the C ABI of include/kp1.h.  Method names, argument meaning and error
behaviour follow the reference class and SB3's VecEnv where the trainers use it
(``env_method("set_curriculum_stage", k)``, auto-reset with ``terminal_observation``).

PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
from typing import Any

import numpy as np
import torch

from . import config as kcfg
from . import native


class _DevView:
    """Expose a raw device pointer to torch through __cuda_array_interface__ (zero copy)."""

    def __init__(self, ptr: int, shape: tuple[int, ...], typestr: str) -> None:
        self.__cuda_array_interface__ = {"data": (int(ptr), False), "shape": tuple(shape), "typestr": typestr, "version": 2, "strides": None}


def _view(ptr: int, shape: tuple[int, ...], typestr: str, device: torch.device) -> torch.Tensor:
    return torch.as_tensor(_DevView(ptr, shape, typestr), device=device)


_stream_arg = native.stream_arg


class DeviceEnvHandle:
    """What the env handle families share: the handle-owned step outputs, ``step`` / ``step_into``, the PCG64 state
    round trip, the reset mask, ``env_method`` and the lifetime.  A family sets ``L``, ``_handle``, ``n_envs``, ``device`` and ``dtype``,
    makes its create call, and supplies the one-line methods that hold its C calls: ``_step_call(*ptrs)``, ``_rng_get_call(arr)``,
    ``_rng_set_call(arr)``, ``_set_obs_stride_call(stride)`` and ``_destroy()``."""

    _typestr = property(lambda self: "<f4" if self.dtype == torch.float32 else "<f8")     # of a _view of the handle's real-typed state

    def _alloc_obs(self, stride: int) -> None:
        self.obs_stride = int(stride)
        self.obs = torch.zeros((self.n_envs, self.obs_stride), dtype=torch.float32, device=self.device)
        self.terminal_obs = torch.zeros_like(self.obs)

    def _alloc_buffers(self, stride: int) -> None:
        """the buffers ``reset`` and ``step`` write: observation rows at pitch ``stride``, reward in the env's real type, done bits"""
        self._alloc_obs(stride)
        self.reward = torch.zeros(self.n_envs, dtype=self.dtype, device=self.device)
        self.done = torch.zeros(self.n_envs, dtype=torch.uint8, device=self.device)

    def set_obs_stride(self, stride: int) -> None:
        """Row pitch of every observation buffer handed to reset / step (the observation width, or the MFMA kernels' zero-padded 64 / 128)."""
        native.check(self._set_obs_stride_call(int(stride)))
        self._alloc_obs(stride)

    def close(self) -> None:
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._destroy()
            self._handle = C.c_void_p()

    def __del__(self) -> None:  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def env_method(self, name: str, *args: Any, **kwargs: Any) -> list[Any]:
        """VecEnv.env_method: the trainers only broadcast (callbacks.py:55,69,162)."""
        result = getattr(self, name)(*args, **kwargs)
        return [result] * self.n_envs

    def _reset_mask(self, mask: torch.Tensor | None) -> torch.Tensor | None:
        """reset(mask=) as contiguous bytes on the handle's device (the caller keeps them alive over the call)"""
        return None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()

    def _host_rows(self, val: Any, width: int, keep: list[np.ndarray]) -> int:
        """address of ``val`` broadcast to [N, width] contiguous float64 rows in host memory, which ``keep`` holds alive over the call"""
        keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(val, dtype=np.float64), (self.n_envs, width))))
        return keep[-1].ctypes.data

    def step(self, actions: torch.Tensor, *, auto_reset: bool = True) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """step(actions[N,7]) -> (obs[N,stride] f32, reward[N], done[N] u8 bitmask).  Finished episodes are reset in the
        same launch (VecEnv semantics); their last observation is in ``self.terminal_obs``."""
        if actions.shape != (self.n_envs, kcfg.NJ):
            raise ValueError(f"Expected action shape {(self.n_envs, kcfg.NJ)}, got {tuple(actions.shape)}")
        self.step_into(actions.to(device=self.device, dtype=self.dtype).contiguous(), self.obs, self.reward, self.done, self.terminal_obs, auto_reset)
        return self.obs, self.reward, self.done

    def step_into(self, actions: torch.Tensor, obs: torch.Tensor, reward: torch.Tensor, done: torch.Tensor,
                  terminal_obs: torch.Tensor | None, auto_reset: bool = True) -> None:
        """Zero-copy variant used by the rollout loop: outputs go straight into caller-owned (rollout) buffers."""
        native.check(self._step_call(native.ptr(actions), native.ptr(obs), native.ptr(reward), native.ptr(done), native.ptr(terminal_obs),
                                     int(auto_reset)))

    def rng_state(self) -> np.ndarray:
        """[N,6] uint64 words (state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger) of each env's PCG64 stream."""
        arr = (kcfg.RngState * self.n_envs)()
        native.check(self._rng_get_call(arr))
        return np.array([[s.state_hi, s.state_lo, s.inc_hi, s.inc_lo, s.has_uint32, s.uinteger] for s in arr], dtype=np.uint64)

    def set_rng_state(self, words: np.ndarray) -> None:
        """the handle's PCG64 streams <- [N, 6] words in rng_state()'s layout"""
        arr = (kcfg.RngState * self.n_envs)()
        for i in range(self.n_envs):
            (arr[i].state_hi, arr[i].state_lo, arr[i].inc_hi, arr[i].inc_lo) = (int(w) for w in words[i][:4])
            arr[i].has_uint32, arr[i].uinteger = int(words[i][4]), int(words[i][5])
        native.check(self._rng_set_call(arr))


class ArmKinematicVecEnv(DeviceEnvHandle):
    """N kinematic_phase1 environments on one MI355X.

    Parameters mirror ``make_vec_env(ArmKinematicEnv, n_envs, seed)``: env ``i`` owns the numpy
    PCG64 stream ``default_rng(seed + first_env_id + i)``.
    """

    metadata = {"render_modes": []}

    def __init__(self, config: kcfg.EnvConfig, n_envs: int, *, device: int | torch.device = 0, seed: int = 0,
                 first_env_id: int = 0, real: str = "f32", reward_components: bool = False) -> None:
        if not torch.cuda.is_available():
            raise native.Kp1Error("ArmKinematicVecEnv needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
        self.L = native.load()
        self.config = config
        self.n_envs = int(n_envs)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.real_type = {"f32": native.REAL_F32, "f64": native.REAL_F64}[real]
        self.dtype = torch.float32 if real == "f32" else torch.float64
        self._handle = C.c_void_p()
        with torch.cuda.device(self.device):
            native.check(self.L.kp1_create(C.byref(config.c), self.n_envs, native.device_index(self.device), self.real_type,
                                           int(seed), int(first_env_id), _stream_arg(self.device), C.byref(self._handle)))
        if config.handoff_states:
            arr = config.handoff_array()
            native.check(self.L.kp1_set_handoff_states(self._handle, C.cast(arr, C.c_void_p), len(config.handoff_states)))
        if config.route_reset.active:
            self.set_route_stride_reset(config.route_reset)
        self._alloc_buffers(kcfg.OBS_DIM)
        self._mode_name = config.mode_name
        # bumped by every setter whose value a captured hipGraph of kp1_step would have frozen into kernel arguments (stage, mode, config,
        # reward-component switch, handoff buffer, observation pitch): ppo.PPO re-captures its rollout graph when it changes
        self.launch_args_version = 0
        if reward_components:
            self.enable_reward_components(True)

    # ------------------------------------------------------------------ the family's C calls behind DeviceEnvHandle
    def _step_call(self, *ptrs: Any) -> int:
        return self.L.kp1_step(self._handle, *ptrs)

    def _rng_get_call(self, arr: Any) -> int:
        return self.L.kp1_rng_get(self._handle, arr)

    def _rng_set_call(self, arr: Any) -> int:
        return self.L.kp1_rng_set(self._handle, arr)

    def _set_obs_stride_call(self, stride: int) -> int:
        return self.L.kp1_set_obs_stride(self._handle, stride)

    def _destroy(self) -> None:
        self.L.kp1_destroy(self._handle)

    # ------------------------------------------------------------------ reference API
    def set_curriculum_stage(self, stage_index: int) -> None:
        native.check(self.L.kp1_set_stage(self._handle, int(stage_index)))
        self.launch_args_version += 1

    def get_curriculum_stage(self) -> int:
        out = C.c_int32()
        native.check(self.L.kp1_get_stage(self._handle, C.byref(out)))
        return int(out.value)

    def set_policy_mode(self, mode_name: str) -> None:
        if mode_name not in kcfg.MODE_NAMES:
            raise ValueError(f"Unsupported policy mode '{mode_name}'")
        native.check(self.L.kp1_set_mode(self._handle, kcfg.MODE_NAMES[mode_name]))
        self._mode_name = mode_name
        self.launch_args_version += 1

    def apply_dock_training_stage(self, stage_updates: dict[str, Any]) -> None:
        """arm_kinematic_env.py:459-487: env scalar + dock_reset overrides for the dock curriculum."""
        if self.config.mode_name != "dock":
            return
        c = self.config.c
        for key, value in dict(stage_updates.get("dock_reset", {})).items():
            if key in ("goal_q", "goal_noise", "init_q_noise", "close_init_q_noise"):
                getattr(c.dock_reset, key)[:] = [float(v) for v in value]
            elif key.startswith("handoff_state_") and key != "handoff_state_probability":
                raise NotImplementedError("changing the handoff buffer filter mid-run: rebuild the EnvConfig instead")
            else:
                if not hasattr(c.dock_reset, key):
                    raise TypeError(f"DockResetConfig.__init__() got an unexpected keyword argument '{key}'")
                setattr(c.dock_reset, key, type(getattr(c.dock_reset, key))(value))
        for key in (
            "action_delta_scale", "dock_action_delta_scale", "dock_residual_action_limit", "dock_delta_q_change_limit_scale",
            "dock_dynamic_action_limit_near_pos_threshold_m", "dock_dynamic_action_limit_far_pos_threshold_m",
            "dock_dynamic_residual_action_limit_near", "dock_dynamic_residual_action_limit_far",
            "dock_dynamic_delta_q_change_limit_scale_near", "dock_dynamic_delta_q_change_limit_scale_far",
        ):
            if key in stage_updates:
                setattr(c.env, key, float(stage_updates[key]))
        native.check(self.L.kp1_update_config(self._handle, C.byref(c)))
        self.launch_args_version += 1

    def set_handoff_states(self, states: list[dict[str, Any]]) -> None:
        """Replace the handoff-state buffer dock resets draw from (reset_samplers.py:131-165).  The old device buffer is freed: a
        rollout graph captured before this call must not be replayed again (PPO checks launch_args_version)."""
        self.config.handoff_states = list(states)
        arr = self.config.handoff_array()
        native.check(self.L.kp1_set_handoff_states(self._handle, C.cast(arr, C.c_void_p), len(self.config.handoff_states)))
        self.launch_args_version += 1

    def set_route_stride_reset(self, route_reset: "kcfg.RouteResetConfig | None") -> None:
        """env.route_reset (reset_samplers.py:393-423): Approach resets draw start and goal from the route, a stage-dependent stride apart.
        ``None``, a disabled block or one without points switches the sampler off.  The handle's sampler block is rewritten in place: a
        captured rollout graph replayed afterwards samples from the new table, and replaced tables live until ``close()``."""
        rr = route_reset if route_reset is not None else kcfg.RouteResetConfig()
        if not rr.active:
            native.check(self.L.kp1_set_route_stride_reset(self._handle, None, 0, None, 0, None, 0, None, None, 0.0))
        else:
            q = (C.c_double * (kcfg.NJ * len(rr.route_q)))(*[v for p in rr.route_q for v in p])
            lo = (C.c_int32 * len(rr.min_stride_by_stage))(*rr.min_stride_by_stage)
            hi = (C.c_int32 * len(rr.max_stride_by_stage))(*rr.max_stride_by_stage)
            sn, gn = (C.c_double * kcfg.NJ)(*rr.start_q_noise), (C.c_double * kcfg.NJ)(*rr.goal_q_noise)
            native.check(self.L.kp1_set_route_stride_reset(self._handle, C.cast(q, C.c_void_p), len(rr.route_q), C.cast(lo, C.c_void_p), len(lo),
                                                           C.cast(hi, C.c_void_p), len(hi), C.cast(sn, C.c_void_p), C.cast(gn, C.c_void_p),
                                                           float(rr.reverse_probability)))
        self.config.route_reset = rr

    def set_obs_stride(self, stride: int) -> None:
        """(56, or 64 = zero-padded for the MFMA GEMMs; the pitch is a kernel argument of kp1_step, hence the bump)"""
        super().set_obs_stride(stride)
        self.launch_args_version += 1

    def seed(self, seed: int, first_env_id: int = 0) -> None:
        native.check(self.L.kp1_seed(self._handle, int(seed), int(first_env_id)))

    def reset(self, *, seed: int | None = None, options: dict[str, Any] | None = None, mask: torch.Tensor | None = None) -> torch.Tensor:
        """reset(seed=, options=) for all envs (or those where mask != 0).  options values are
        [N,7] / [N,6] arrays (or a single row, broadcast), like the reference's per-env dict."""
        if seed is not None:
            self.seed(seed)
        opts_p = None
        keep: list[np.ndarray] = []
        if options:
            o = kcfg.ResetOpts()
            o.policy_mode = -1
            for key, width in (("initial_q", 7), ("initial_dq", 7), ("initial_prev_action", 7), ("goal_q", 7), ("goal_pose6", 6)):
                val = options.get(key)
                if val is None:
                    continue
                arr = np.asarray(val, dtype=np.float64)
                shape = (self.n_envs, arr.shape[0]) if arr.ndim == 1 else arr.shape      # one row stands for every env
                if shape != (self.n_envs, width):
                    raise ValueError(f"options['{key}'] must have shape ({self.n_envs}, {width}), got {shape}")
                setattr(o, key, self._host_rows(arr, width, keep))
            pm = options.get("policy_mode")
            if pm is not None:
                if pm not in kcfg.MODE_NAMES:
                    raise ValueError(f"Unsupported policy mode '{pm}'")
                o.policy_mode = kcfg.MODE_NAMES[pm]
                self._mode_name = pm
            opts_p = C.byref(o)
        else:
            self._mode_name = self.config.mode_name
        mask = self._reset_mask(mask)
        native.check(self.L.kp1_reset(self._handle, native.ptr(mask), opts_p, native.ptr(self.obs)))
        return self.obs

    def use_current_stream(self) -> None:
        """Order this handle's launches on torch's current stream (call inside torch.cuda.graph capture / stream contexts)."""
        native.check(self.L.kp1_set_stream(self._handle, _stream_arg(self.device)))

    def snapshot(self) -> None:
        """Device-side copy of the whole env state (all fields, counters and PCG64 streams), ordered on the handle's stream."""
        native.check(self.L.kp1_state_snapshot(self._handle))

    def restore(self) -> None:
        """Put the state of the last snapshot() back (episodes and random streams continue exactly from there)."""
        native.check(self.L.kp1_state_restore(self._handle))

    def current_observation(self) -> torch.Tensor:
        out = torch.empty_like(self.obs)
        native.check(self.L.kp1_observe(self._handle, native.ptr(out)))
        return out

    @staticmethod
    def obs_dict(obs: torch.Tensor) -> dict[str, torch.Tensor]:
        """Split [N,56] into the reference's 13-key Dict observation (views)."""
        return {k: obs[..., s:s + n] for k, (s, n) in kcfg.OBS_LAYOUT.items()}

    # ------------------------------------------------------------------ info / state
    def info(self) -> dict[str, torch.Tensor]:
        """Device views of the info keys downstream code reads (arm_kinematic_env.py:384-423)."""
        v = kcfg.InfoView()
        native.check(self.L.kp1_get_info(self._handle, C.byref(v)))
        n, ts, dev = self.n_envs, self._typestr, self.device
        out = {
            "position_error_norm": _view(v.position_error_norm, (n,), ts, dev),
            "orientation_error_norm": _view(v.orientation_error_norm, (n,), ts, dev),
            "min_position_error": _view(v.min_position_error, (n,), ts, dev),
            "executed_delta_q_l2": _view(v.executed_delta_q_l2, (n,), ts, dev),
            "action_l2": _view(v.action_l2, (n,), ts, dev),
            "delta_q_change_l2": _view(v.delta_q_change_l2, (n,), ts, dev),
            "q": _view(v.q, (7, n), ts, dev), "dq": _view(v.dq, (7, n), ts, dev),
            "prev_action": _view(v.prev_action, (7, n), ts, dev), "goal_q": _view(v.goal_q, (7, n), ts, dev),
            "goal_pose6": _view(v.goal_pose6, (6, n), ts, dev), "ee_pose6": _view(v.ee_pose6, (6, n), ts, dev),
            "entry_metrics": _view(v.entry_metrics, (4, n), ts, dev),
            "step_count": _view(v.episode_step, (n,), "<i4", dev), "dwell_count": _view(v.dwell_count, (n,), "<i4", dev),
            "near_goal_entry_count": _view(v.near_goal_entry_count, (n,), "<i4", dev),
            "near_goal_drift_count": _view(v.near_goal_drift_count, (n,), "<i4", dev),
            "flags": _view(v.flags, (n,), "<i4", dev), "stage_index": _view(v.stage_index, (n,), "<i4", dev),
        }
        return out

    def enable_reward_components(self, enable: bool = True) -> None:
        native.check(self.L.kp1_enable_reward_components(self._handle, int(enable)))
        self._reward_components_on = bool(enable)
        self.launch_args_version += 1

    def reward_components(self) -> tuple[list[str], torch.Tensor]:
        ptr, n = C.c_void_p(), C.c_int32()
        native.check(self.L.kp1_get_reward_components(self._handle, C.byref(ptr), C.byref(n)))
        mode = kcfg.MODE_NAMES[self._mode_name]
        return native.component_names(mode), _view(ptr.value, (int(n.value), self.n_envs), self._typestr, self.device)

    def get_state(self) -> dict[str, np.ndarray]:
        n = self.n_envs
        out = {k: np.empty((n, 6 if k == "goal_pose6" else 7)) for k in ("q", "dq", "prev_action", "goal_q", "goal_pose6")}
        native.check(self.L.kp1_get_state(self._handle, *[out[k].ctypes.data for k in ("q", "dq", "prev_action", "goal_q", "goal_pose6")]))
        return out

    def set_state(self, *, q=None, dq=None, prev_action=None, goal_q=None, goal_pose6=None, capture_entry_metrics: bool = True) -> None:
        keep: list[np.ndarray] = []
        ptrs = [None if val is None else self._host_rows(val, w, keep) for val, w in ((q, 7), (dq, 7), (prev_action, 7), (goal_q, 7), (goal_pose6, 6))]
        native.check(self.L.kp1_set_state(self._handle, *ptrs, int(capture_entry_metrics)))


class ReplicaEnv:
    """Replica k of a population handle: the attributes PPO's setup, ReplicaView, ``checkpoint.save`` and the evaluators read.  Stepping and
    resetting go through the population handle (one launch for all replicas).  A family's view adds what only that family has."""

    def __init__(self, pop: Any, k: int) -> None:
        self.pop, self.k = pop, int(k)
        self.n_envs = pop.n_per_replica
        self.device, self.dtype, self.config = pop.device, pop.dtype, pop.config
        self.obs_dim = getattr(pop, "obs_dim", kcfg.OBS_DIM)
        self.seed = pop.seeds[self.k]

    @property
    def launch_args_version(self) -> int:
        return self.pop.launch_args_version

    @property
    def obs_stride(self) -> int:
        return self.pop.obs_stride

    def set_obs_stride(self, stride: int) -> None:
        if int(stride) != self.pop.obs_stride:
            self.pop.set_obs_stride(stride)

    def use_current_stream(self) -> None:
        self.pop.use_current_stream()

    def reset(self, **_: Any) -> torch.Tensor:
        name = type(self.pop).__name__
        raise TypeError(f"a replica of {'an' if name[0] in 'AEIOU' else 'a'} {name} is reset through the population handle (one reset of all replicas)")

    def close(self) -> None:
        """(the population handle owns the envs)"""


class ArmKinematicReplicaEnv(ReplicaEnv):
    """Replica k of an ArmKinematicPopulationVecEnv.  It has ``snapshot`` / ``restore``, by which PPO rolls a graph warm-up back (a view
    without them gets a fresh reset): the whole population handle's, so every replica's view takes the same snapshot."""

    def snapshot(self) -> None:
        self.pop.snapshot()

    def restore(self) -> None:
        self.pop.restore()


class PopulationEnvHandle:
    """The population half of an env handle, in front of the family's single class (``class XPopulationVecEnv(PopulationEnvHandle, XVecEnv)``):
    K replicas of ``n_per_replica`` envs each in ONE handle, block k = rows [k N, (k + 1) N), created with per-block seeds that it keeps.
    The family's constructor calls ``_take_seeds``, makes the refusals of its own, calls ``_take_blocks`` and creates its handle with
    ``seeds[0]`` before it seeds the blocks; ``replica_type`` is its view."""

    replica_type: type = ReplicaEnv

    def _take_seeds(self, seeds: Any) -> None:
        self.seeds = [int(s) for s in seeds]
        if not self.seeds:
            raise ValueError(f"{type(self).__name__} needs at least one seed")

    def _take_blocks(self, n_per_replica: int) -> int:
        """-> the handle's env count K N"""
        self.K = len(self.seeds)
        self.n_per_replica = int(n_per_replica)
        if self.n_per_replica < 1:
            raise ValueError("n_per_replica must be positive")
        return self.K * self.n_per_replica

    def replica(self, k: int) -> ReplicaEnv:
        if not 0 <= int(k) < self.K:
            raise IndexError(f"replica {k} of a population of {self.K}")
        return self.replica_type(self, int(k))

    def rows(self, k: int) -> slice:
        return slice(k * self.n_per_replica, (k + 1) * self.n_per_replica)

    def seed(self, seed: int, first_env_id: int = 0) -> None:
        raise ValueError("a population env keeps the per-block seeds it was created with (env i of replica k: seeds[k] + i)")


MAX_REPLICAS = native.header_int("KP1_CURRICULUM_MAX_REPLICAS")     # = KP1_MLP_MAX_REPLICAS


class ArmKinematicPopulationVecEnv(PopulationEnvHandle, ArmKinematicVecEnv):
    """K Approach or Finisher (dock-mode) envs of ``n_per_replica`` envs each in ONE handle: block k = rows [k N, (k + 1) N) is replica k, and
    is bit for bit ``ArmKinematicVecEnv(config, n_per_replica, seed=seeds[k])`` (env i of replica k owns ``default_rng(seeds[k] + i)``,
    kp1_seed_blocks; with ``repeated_seeds=True`` seeds may repeat -- a hyper-parameter sweep runs several replicas on one seed -- and equal
    seeds give equal env streams).  One ``step_into`` covers all K N rows, so a population rollout is one env step launch per step whatever K is -- the
    [K N, obs_w] buffers are the population rollout's replica-major layout.

    Approach: a PointCurriculumPopulation attached to it gives every replica its own curriculum stage: the auto-reset of env i reads the stage
    of tracker i / N (the population form of the step kernel).  ``reset()`` uses the handle's host stage, which K single handles made from one
    config share.  Dock: a DockReverseCurriculumPopulation gives every replica its own reverse-curriculum stage; the step and ``reset()`` of
    env i read what a stage overrides from replica i / N's live stage record, and the shared config is never rewritten by a promotion.
    Without a tracker a dock population is the plain dock step over K N envs.  ``mode`` names the config's mode ("approach" by default, "dock"
    for a Finisher population).  f32 only; the handle keeps its per-block seeds (``seed()`` is refused) and runs its config's mode.  ``replica(k)`` is a view with what PPO's setup, ReplicaView and ``checkpoint.save`` read."""

    is_population = True
    replica_type = ArmKinematicReplicaEnv

    def __init__(self, config: kcfg.EnvConfig, seeds: list[int], n_per_replica: int, *, device: int | torch.device = 0, real: str = "f32",
                 reward_components: bool = False, mode: str = "approach", repeated_seeds: bool = False) -> None:
        self._take_seeds(seeds)
        if len(self.seeds) > MAX_REPLICAS:
            raise ValueError(f"ArmKinematicPopulationVecEnv holds at most {MAX_REPLICAS} replicas (got {len(self.seeds)} seeds)")
        if not repeated_seeds and len(set(self.seeds)) != len(self.seeds):
            raise ValueError(f"ArmKinematicPopulationVecEnv seeds must be distinct (got {self.seeds}); a hyper-parameter sweep that runs several "
                             "replicas on one seed passes repeated_seeds=True")
        if mode not in ("approach", "dock"):
            raise ValueError(f"ArmKinematicPopulationVecEnv runs the Approach or the dock mode, not {mode!r}")
        if config.mode_name != mode:
            raise ValueError(f"ArmKinematicPopulationVecEnv(mode={mode!r}) got a {config.mode_name}-mode config: a dock-mode population is asked for "
                             "with mode='dock' (its per-replica stages come from a DockReverseCurriculumPopulation, not from K DockReverseCurriculum)")
        if real != "f32":
            raise ValueError("ArmKinematicPopulationVecEnv is the f32 env (the population step kernel has no f64 form)")
        super().__init__(config, self._take_blocks(n_per_replica), device=device, seed=self.seeds[0], real="f32", reward_components=reward_components)
        seeds_c = (C.c_uint64 * self.K)(*self.seeds)
        native.check(self.L.kp1_seed_blocks(self._handle, C.cast(seeds_c, C.c_void_p), self.K, self.n_per_replica))
        self.dock_population: Any = None     # the DockReverseCurriculumPopulation attached to a dock-mode population

    def set_policy_mode(self, mode_name: str) -> None:
        if mode_name != self.config.mode_name:
            raise ValueError(f"a population env runs its config's mode ({self.config.mode_name}) only")
        super().set_policy_mode(mode_name)

    def reset(self, *, seed: int | None = None, options: dict[str, Any] | None = None, mask: torch.Tensor | None = None) -> torch.Tensor:
        if options and options.get("policy_mode") not in (None, self.config.mode_name):
            raise ValueError(f"a population env runs its config's mode ({self.config.mode_name}) only")
        return super().reset(seed=seed, options=options, mask=mask)

    def apply_dock_training_stage(self, stage_updates: dict[str, Any]) -> None:
        if self.dock_population is not None:
            raise ValueError("a DockReverseCurriculumPopulation is attached: each replica's stage lives in its own live record, and a "
                             "stage applied to the shared config would reach no replica")
        super().apply_dock_training_stage(stage_updates)


def fk_pose6(q: torch.Tensor) -> torch.Tensor:
    """compute_ee_pose6 batched on the GPU (kinematics/fk_interface.py:21-22): q[n,7] -> pose6[n,6]."""
    if q.ndim != 2 or q.shape[1] != kcfg.NJ:
        raise ValueError("Expected q of shape (n, 7)")
    if not q.is_cuda:
        raise native.Kp1Error("fk_pose6 needs a device tensor; there is no CPU fallback")
    rt = _real_type(q)
    q = q.contiguous()
    out = torch.empty((q.shape[0], 6), dtype=q.dtype, device=q.device)
    native.check(native.load().kp1_fk_pose6(native.device_index(q.device), rt, native.ptr(q), native.ptr(out), q.shape[0], _stream_arg(q.device)))
    return out


def _real_type(t: torch.Tensor) -> int:
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError("expected a float32 or float64 tensor")
    if not t.is_cuda:
        raise native.Kp1Error("needs a device tensor; there is no CPU fallback")
    return native.REAL_F64 if t.dtype == torch.float64 else native.REAL_F32


def pose_error_components(curr_pose6: torch.Tensor, goal_pose6: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """kinematics/pose_utils.py:21-30 batched on the GPU through the device function of the step kernel:
    (pos_err[n,3], ori_err[n,3] wrapped per component to [-pi, pi), norms[n,2])."""
    if curr_pose6.shape != goal_pose6.shape or curr_pose6.ndim != 2 or curr_pose6.shape[1] != 6 or curr_pose6.dtype != goal_pose6.dtype:
        raise ValueError("Expected two pose6 tensors of shape (n, 6) and equal dtype")
    rt = _real_type(curr_pose6)
    c, g = curr_pose6.contiguous(), goal_pose6.contiguous()
    n = c.shape[0]
    pe, oe, nr = (torch.empty((n, k), dtype=c.dtype, device=c.device) for k in (3, 3, 2))
    native.check(native.load().kp1_pose_error(native.device_index(c.device), rt, native.ptr(c), native.ptr(g), native.ptr(pe), native.ptr(oe), native.ptr(nr), n,
                                              _stream_arg(c.device)))
    return pe, oe, nr


def joint_utils(config: kcfg.EnvConfig, q: torch.Tensor, dq: torch.Tensor) -> dict[str, torch.Tensor]:
    """kinematics/joint_limits.py:133-174 batched on the GPU through the device functions of the hot path:
    clipped = clip(q), margin = joint_limit_margin(clipped), q_norm = normalize_joint_positions(q), dq_norm = normalize_joint_deltas(dq)."""
    if q.shape != dq.shape or q.ndim != 2 or q.shape[1] != kcfg.NJ or q.dtype != dq.dtype:
        raise ValueError("Expected q and dq of shape (n, 7) and equal dtype")
    rt = _real_type(q)
    q, dq = q.contiguous(), dq.contiguous()
    out = {k: torch.empty_like(q) for k in ("clipped", "margin", "q_norm", "dq_norm")}
    native.check(native.load().kp1_joint_utils(native.device_index(q.device), rt, C.byref(config.c), native.ptr(q), native.ptr(dq),
                                               *(native.ptr(out[k]) for k in ("clipped", "margin", "q_norm", "dq_norm")), q.shape[0],
                                               _stream_arg(q.device)))
    return out
