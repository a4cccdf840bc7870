"""Device-resident PointCurriculumCallback (reference: kinematic_phase1/training/callbacks.py:32-101).

The reference callback runs on the host after every VecEnv step.  Here the same per-episode rule runs as a
one-wave HIP kernel on the rollout stream (include/kp1_ppo.h), so a 4096-env rollout never synchronises with
the host; the env kernel reads the published stage from device memory.  ``summary()`` mirrors the reference's.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Sequence

import torch

from . import native

MAX_WINDOW = native.header_int("KP1_CURRICULUM_MAX_WINDOW")
MAX_HISTORY = native.header_int("KP1_CURRICULUM_MAX_HISTORY")


class _Event(C.Structure):
    _fields_ = [("total_timesteps", C.c_int64), ("from_stage", C.c_int32), ("to_stage", C.c_int32), ("trigger_success_rate", C.c_double)]


class CurriculumState(C.Structure):
    _fields_ = [
        ("stage_index", C.c_int32), ("stage_episode_count", C.c_int32), ("ring_len", C.c_int32), ("ring_head", C.c_int32),
        ("window_episodes", C.c_int32), ("min_episodes_per_stage", C.c_int32), ("max_stage_index", C.c_int32), ("n_events", C.c_int32),
        ("success_rate_threshold", C.c_double), ("num_timesteps", C.c_int64),
        ("ring", C.c_int32 * MAX_WINDOW), ("events", _Event * MAX_HISTORY),
    ]


class PointCurriculum:
    def __init__(self, *, success_rate_threshold: float, window_episodes: int, min_episodes_per_stage: int, max_stage_index: int,
                 initial_stage_index: int = 0, device: torch.device | int = 0) -> None:
        self.L = native.load()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._st = C.c_void_p()
        native.check(self.L.kp1_curriculum_create(self.device.index or 0, float(success_rate_threshold), int(window_episodes),
                                                  int(min_episodes_per_stage), int(max_stage_index), int(initial_stage_index), C.byref(self._st)))

    @property
    def stage_ptr(self) -> int:
        """device address of the int32 current stage (first word of the state)"""
        return int(self._st.value)

    @property
    def device_state(self) -> int:
        """device address of the tracker state (a PointCurriculumPopulation: of its K contiguous states), what kp1_rollout_run takes as
        ``trackers``"""
        return int(self._st.value)

    def attach(self, env) -> None:
        """_on_training_start: the envs follow this tracker's stage from now on (callbacks.py:68-69)."""
        native.check(self.L.kp1_bind_stage_ptr(env._handle, C.c_void_p(self.stage_ptr)))

    def observe(self, dones: torch.Tensor, steps_per_call: int) -> None:
        stream = torch.cuda.current_stream(self.device).cuda_stream
        native.check(self.L.kp1_curriculum_observe(self.device.index or 0, self._st, C.c_void_p(dones.data_ptr()), int(dones.numel()),
                                                   int(steps_per_call), C.c_void_p(stream)))

    def observe_chunk(self, dones_all: torch.Tensor, n_local: int, chunk_steps: int, world: int) -> None:
        """data-parallel rollouts: the all-gathered [world, chunk_steps, n_local] done bytes of a chunk of env steps, replayed in the
        reference's order (step by step, global env id order inside a step)"""
        assert dones_all.numel() == world * chunk_steps * n_local and dones_all.dtype == torch.uint8 and dones_all.is_contiguous()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        native.check(self.L.kp1_curriculum_observe_chunk(self.device.index or 0, self._st, C.c_void_p(dones_all.data_ptr()), int(n_local), int(chunk_steps),
                                                         int(world), C.c_void_p(stream)))

    def read(self) -> CurriculumState:
        out = CurriculumState()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        native.check(self.L.kp1_curriculum_read(self.device.index or 0, self._st, C.byref(out), C.c_void_p(stream)))
        return out

    def summary(self) -> dict[str, object]:
        """callbacks.py:94-101"""
        return self._summary_of(self.read())

    @staticmethod
    def _summary_of(st: CurriculumState) -> dict[str, object]:
        n = st.ring_len
        recent = [st.ring[k] for k in range(n)]
        return {
            "stage_index": int(st.stage_index),
            "stage_episode_count": int(st.stage_episode_count),
            "recent_success_rate": float(sum(recent)) / float(n) if n else 0.0,
            "history": [
                {"from_stage_index": int(e.from_stage), "to_stage_index": int(e.to_stage),
                 "trigger_success_rate": float(e.trigger_success_rate), "total_timesteps": int(e.total_timesteps)}
                for e in list(st.events)[: min(st.n_events, MAX_HISTORY)]
            ],
        }

    def close(self) -> None:
        if self._st.value:
            self.L.kp1_curriculum_destroy(self.device.index or 0, self._st)
            self._st = C.c_void_p()


class PointCurriculumPopulation(PointCurriculum):
    """K device trackers, one per replica of an ArmKinematicPopulationVecEnv (include/kp1_ppo.h, kp1_curriculum_*_population): tracker k
    starts on ``initial_stage_indices[k]``, the other settings are shared.  ONE ``observe(dones[K N])`` launch per env step: workgroup k
    replays replica k's done bytes into tracker k by PointCurriculum's rule.  ``attach(env)`` makes env i of the population auto-reset on
    tracker i / N's stage.  ``read(k)`` / ``summary(k)`` are PointCurriculum's of replica k; ``replica(k)`` is a view with read() /
    summary() for the per-replica lists of a population run.  There is no data-parallel (chunk) form."""

    def __init__(self, *, success_rate_threshold: float, window_episodes: int, min_episodes_per_stage: int, max_stage_index: int,
                 initial_stage_indices: Sequence[int], device: torch.device | int = 0) -> None:
        from .vec_env import MAX_REPLICAS

        stages = [int(s) for s in initial_stage_indices]
        if not 1 <= len(stages) <= MAX_REPLICAS:
            raise ValueError(f"PointCurriculumPopulation holds 1 to {MAX_REPLICAS} trackers (got {len(stages)} initial stages)")
        self.K = len(stages)
        self.env: Any = None
        self.L = native.load()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._st = C.c_void_p()
        init = (C.c_int32 * self.K)(*stages)
        native.check(self.L.kp1_curriculum_create_population(self.device.index or 0, self.K, float(success_rate_threshold), int(window_episodes),
                                                             int(min_episodes_per_stage), int(max_stage_index), C.cast(init, C.c_void_p),
                                                             C.byref(self._st)))

    @property
    def stage_ptr(self) -> int:
        raise TypeError("a population tracker has one stage per replica: attach() binds all of them to a population env")

    def attach(self, env: Any) -> None:
        """_on_training_start of every replica: env i of the population auto-resets on tracker i / N's stage from now on"""
        if not getattr(env, "is_population", False):
            raise TypeError("PointCurriculumPopulation tracks the replicas of an ArmKinematicPopulationVecEnv")
        if env.n_envs % self.K != 0 or getattr(env, "K", self.K) != self.K:
            raise ValueError(f"a population env of {env.n_envs} envs does not split into this tracker's {self.K} replicas")
        native.check(self.L.kp1_bind_population_stages(env._handle, C.c_void_p(self._st.value), self.K))
        env.launch_args_version += 1     # a captured rollout froze the step kernel (and its stage source) into the graph
        self.env = env

    def observe(self, dones: torch.Tensor, steps_per_call: int) -> None:
        """dones: the K N done bytes of one population step (replica-major); steps_per_call: env steps per replica this call stands for (N)"""
        if dones.numel() % self.K != 0 or dones.dtype != torch.uint8 or not dones.is_contiguous():
            raise ValueError(f"observe() takes the contiguous uint8 done bytes of all {self.K} replicas")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        native.check(self.L.kp1_curriculum_observe_population(self.device.index or 0, self._st, C.c_void_p(dones.data_ptr()), dones.numel() // self.K,
                                                              self.K, int(steps_per_call), C.c_void_p(stream)))

    def observe_chunk(self, dones_all: torch.Tensor, n_local: int, chunk_steps: int, world: int) -> None:
        raise TypeError("the population tracker has no data-parallel form")

    def read(self, k: int = 0) -> CurriculumState:
        out = CurriculumState()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        native.check(self.L.kp1_curriculum_read_replica(self.device.index or 0, self._st, self.K, int(k), C.byref(out), C.c_void_p(stream)))
        return out

    def summary(self, k: int = 0) -> dict[str, object]:
        return self._summary_of(self.read(k))

    def replica(self, k: int) -> "PointCurriculumReplica":
        if not 0 <= int(k) < self.K:
            raise IndexError(f"replica {k} of a population of {self.K}")
        return PointCurriculumReplica(self, int(k))


class PointCurriculumReplica:
    """Replica k of a PointCurriculumPopulation: read() / summary() of its tracker.  The population observes all replicas at once."""

    def __init__(self, pop: PointCurriculumPopulation, k: int) -> None:
        self.pop, self.k = pop, int(k)

    def attach(self, env: Any) -> None:
        """(the population tracker is attached to the population env)"""

    def observe(self, dones: torch.Tensor, steps_per_call: int) -> None:
        raise TypeError("replica trackers are observed through PointCurriculumPopulation.observe (one launch for all replicas)")

    def read(self) -> CurriculumState:
        return self.pop.read(self.k)

    def summary(self) -> dict[str, object]:
        return self.pop.summary(self.k)
