"""Device-resident PointCurriculumCallback (reference: kinematic_phase1/training/callbacks.py:32-101).

The reference callback runs on the host after every VecEnv step.  Here the same per-episode rule runs as a
one-wave HIP kernel on the rollout stream (include/kp1_ppo.h), so a 4096-env rollout never synchronises with
the host; the env kernel reads the published stage from device memory.  ``summary()`` mirrors the reference's.

``DeviceTracker``, ``TrackerPopulation`` and ``TrackerReplica`` are the Python half that the three device trackers share (this one, the
dock reverse curriculum of finisher_tools.py and the route prefix curriculum of route_curriculum.py): DESIGN.md section 44.
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


def window_mean(st: C.Structure, ring: Any) -> float:
    """mean of the live window of a tracker state: the ``ring_len`` newest outcomes of ``ring``, a ring of ``window_episodes`` slots whose
    oldest live slot is ``ring_head`` (0 while the ring is still filling)"""
    n, cap, head = int(st.ring_len), int(st.window_episodes), int(st.ring_head)
    return float(sum(int(ring[(head + j) % cap]) for j in range(n))) / float(n) if n else 0.0


class DeviceTracker:
    """What a device curriculum tracker's host handle does whatever its family.  A family supplies ``State`` (the ctypes mirror of its device
    state), ``_read_call(k, out, stream)`` (its read entry point, a population's read-replica; returns the status), ``_summary_of(state)``
    and ``_destroy()``, and ``_follow`` where a read has a host-side effect; create, attach and the observe calls stay with the family.
    Nothing here needs ``__init__`` to have run."""

    # PPO's data-parallel rollout exchanges per-step episode records (record / observe_chunk) for this tracker instead of the done bytes
    needs_episode_records = False
    # kp1_rollout_run runs this tracker's step inside the whole-rollout launch (ppo.rollout_run_covered)
    runs_in_rollout_launch = False
    env: Any = None

    def _device(self) -> torch.device:
        return self.env.device

    def _stream(self) -> C.c_void_p:
        """the current stream of the tracker's device: what every launch and read of the tracker is ordered on"""
        return native.stream_arg(self._device())

    def _follow(self, st: Any, k: int) -> None:
        """what the host side keeps in step with the state just read (nothing here)"""

    def _read_state(self, k: int = 0) -> Any:
        out = self.State()
        native.check(self._read_call(int(k), C.byref(out), self._stream()))
        return out

    def read(self, k: int = 0) -> Any:
        """the device state (a population: of tracker ``k``), after the stream's work so far"""
        st = self._read_state(k)
        self._follow(st, int(k))
        return st

    def summary(self, k: int = 0) -> dict[str, object]:
        """the reference callback's ``summary()``"""
        return self._summary_of(self.read(k))

    def close(self) -> None:
        if self._st.value:
            self._destroy()
            self._st = C.c_void_p()


class TrackerPopulation:
    """The population half, mixed in in front of the family's single tracker: K trackers behind one handle, observed by ONE launch per env
    step and read per replica.  ``K`` is the family's (an attribute, or the attached env's)."""

    needs_episode_records = False

    def replica(self, k: int) -> "TrackerReplica":
        if not 0 <= int(k) < self.K:
            raise IndexError(f"replica {k} of a population of {self.K}")
        return TrackerReplica(self, int(k))

    def _check_done_bytes(self, dones: torch.Tensor, count_ok: bool) -> None:
        if not count_ok or dones.dtype != torch.uint8 or not dones.is_contiguous():
            raise ValueError(f"observe() takes the contiguous uint8 done bytes of all {self.K} replicas")

    def record(self, dones: torch.Tensor, out: torch.Tensor) -> None:
        raise TypeError(f"{type(self).__name__} has no data-parallel form (record)")

    def observe_chunk(self, dones_all: torch.Tensor, n_local: int, chunk_steps: int, world: int) -> None:
        raise TypeError(f"{type(self).__name__} has no data-parallel form (observe_chunk)")


class TrackerReplica:
    """Replica k of a tracker population: read() / summary() / current_stage_index of its tracker, and what the population keeps per
    replica or for all of them (``config``: the dock population's EnvConfig copy that read() keeps in step; ``stages``).  The population is
    attached, observed (all replicas at once) and closed; the view does none of that."""

    def __init__(self, pop: Any, k: int) -> None:
        self.pop, self.k = pop, int(k)

    stages = property(lambda self: self.pop.stages)
    config = property(lambda self: self.pop.configs[self.k])
    current_stage_index = property(lambda self: int(self.read().stage_index))

    def attach(self, env: Any) -> None:
        """(the population tracker is attached to the population env)"""

    def observe(self, dones: torch.Tensor, steps_per_call: int) -> None:
        raise TypeError(f"replica trackers are observed through {type(self.pop).__name__}.observe (one launch for all replicas)")

    def read(self) -> Any:
        return self.pop.read(self.k)

    def summary(self) -> dict[str, object]:
        return self.pop.summary(self.k)

    def close(self) -> None:
        """(the population tracker owns the device state)"""


class PointCurriculum(DeviceTracker):
    State = CurriculumState
    runs_in_rollout_launch = True

    def __init__(self, *, success_rate_threshold: float, window_episodes: int, min_episodes_per_stage: int, max_stage_index: int,
                 initial_stage_index: int = 0, device: torch.device | int = 0) -> None:
        self.L = native.load()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._st = C.c_void_p()
        native.check(self.L.kp1_curriculum_create(native.device_index(self.device), float(success_rate_threshold), int(window_episodes),
                                                  int(min_episodes_per_stage), int(max_stage_index), int(initial_stage_index), C.byref(self._st)))

    def _device(self) -> torch.device:
        return self.device

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
        native.check(self.L.kp1_curriculum_observe(native.device_index(self.device), self._st, native.ptr(dones), int(dones.numel()),
                                                   int(steps_per_call), self._stream()))

    def observe_chunk(self, dones_all: torch.Tensor, n_local: int, chunk_steps: int, world: int) -> None:
        """data-parallel rollouts: the all-gathered [world, chunk_steps, n_local] done bytes of a chunk of env steps, replayed in the
        reference's order (step by step, global env id order inside a step)"""
        assert dones_all.numel() == world * chunk_steps * n_local and dones_all.dtype == torch.uint8 and dones_all.is_contiguous()
        native.check(self.L.kp1_curriculum_observe_chunk(native.device_index(self.device), self._st, native.ptr(dones_all), int(n_local), int(chunk_steps),
                                                         int(world), self._stream()))

    def _read_call(self, k: int, out: Any, stream: C.c_void_p) -> int:
        return self.L.kp1_curriculum_read(native.device_index(self.device), self._st, out, stream)

    @staticmethod
    def _summary_of(st: CurriculumState) -> dict[str, object]:
        """callbacks.py:94-101"""
        return {
            "stage_index": int(st.stage_index),
            "stage_episode_count": int(st.stage_episode_count),
            "recent_success_rate": window_mean(st, st.ring),
            "history": [
                {"from_stage_index": int(e.from_stage), "to_stage_index": int(e.to_stage),
                 "trigger_success_rate": float(e.trigger_success_rate), "total_timesteps": int(e.total_timesteps)}
                for e in list(st.events)[: min(st.n_events, MAX_HISTORY)]
            ],
        }

    def _destroy(self) -> None:
        self.L.kp1_curriculum_destroy(native.device_index(self.device), self._st)


class PointCurriculumPopulation(TrackerPopulation, PointCurriculum):
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
        native.check(self.L.kp1_curriculum_create_population(native.device_index(self.device), self.K, float(success_rate_threshold), int(window_episodes),
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
        self._check_done_bytes(dones, dones.numel() % self.K == 0)
        native.check(self.L.kp1_curriculum_observe_population(native.device_index(self.device), self._st, native.ptr(dones), dones.numel() // self.K,
                                                              self.K, int(steps_per_call), self._stream()))

    def _read_call(self, k: int, out: Any, stream: C.c_void_p) -> int:
        return self.L.kp1_curriculum_read_replica(native.device_index(self.device), self._st, self.K, k, out, stream)


PointCurriculumReplica = TrackerReplica
