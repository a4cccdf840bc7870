"""The argument refusals of csrc/kp1_ppo.hip that stand in front of its device selection, without a GPU: the GAE scans, the permutation and
advantage statistics, the time-limit bootstrap, the point-curriculum tracker, the training monitor and kp1_explained_variance.  Every case
changes a call that would be accepted in one place (or, for the order of two adjacent checks, in two) and expects KP1_ERR_INVALID with the
exact kp1_last_error() text; the call returns before any HIP call, so a host buffer stands for every device pointer and for the monitor handle.
The two refusals behind the device selection (a window above KP1_CURRICULUM_MAX_WINDOW, a device index out of range) are in
test_ppo_tail_kernels_gpu.py."""
from __future__ import annotations

import ctypes as C

import pytest

from rl_brain_trainer_amd import native

KP1_ERR_INVALID = -1
MAX_REPLICAS = native.header_int("KP1_CURRICULUM_MAX_REPLICAS")
_HOST = (C.c_char * 256)()                       # zeros: as a monitor handle it has K = 0 and max_steps = 0, so every replica and every T is out of range
P = C.cast(_HOST, C.c_void_p).value
OUT = C.pointer(C.c_void_p())                    # kp1_curriculum_state** / kp1_monitor**
STATE = C.pointer(native.MonitorState())

# name -> (an argument list the checks in front of the device selection accept; never passed as it stands,
#          [(case, {argument index: value}, expected text)])
GAE = "bad argument to kp1_gae_scan"
GAE_R = "bad argument to kp1_gae_scan_replicas"
GAE_R_N = "kp1_gae_scan_replicas: N must be a multiple of n_per_replica"
PERM = "bad argument to kp1_random_permutation"
STATS = "bad argument to kp1_adv_minibatch_stats"
SUMS = "bad argument to kp1_adv_minibatch_sums"
BOOT = "bad argument to kp1_bootstrap_truncated"
NULL = "NULL argument"
REPLICAS = "n_replicas must be in [1, KP1_CURRICULUM_MAX_REPLICAS]"
OBS = "bad argument to kp1_curriculum_observe"
CHUNK = "bad argument to kp1_curriculum_observe_chunk"
POP = "bad argument to kp1_curriculum_observe_population"
REPLICA = "replica index out of range"
M_NULL = "kp1_monitor_create: NULL argument"
M_REPLICAS = "kp1_monitor_create: n_replicas must be in [1, KP1_CURRICULUM_MAX_REPLICAS]"
M_PER = "kp1_monitor_create: n_per_replica must be at least 1"
M_WINDOW = "kp1_monitor_create: window must be in [1, KP1_MONITOR_MAX_WINDOW]"
M_STEPS = "kp1_monitor_create: max_steps must be in [1, KP1_MONITOR_MAX_STEPS]"
M_TOTAL = "kp1_monitor_create: max_steps * n_replicas * n_per_replica must stay below 2^31"
MO_NULL = "kp1_monitor_observe: NULL argument"
MO_T = "kp1_monitor_observe: T must be in [1, max_steps of the handle]"
MR_NULL = "kp1_monitor_read: NULL argument"
MR_REPLICA = "kp1_monitor_read: replica index out of range"
EV_NULL = "kp1_explained_variance: NULL argument"
EV_SHAPE = "kp1_explained_variance: T and n_total must be positive and n_total a multiple of n_per_replica"
EV_TOTAL = "kp1_explained_variance: T * n_total must stay below 2^31"


def _each(indices, value, text):
    return [(f"arg{i}={value}", {i: value}, text) for i in indices]


TABLE = {
    "kp1_gae_scan": ([0, P, P, P, P, 0.99, 0.95, P, P, 4, 8, None],
                     _each((1, 2, 3, 4, 7, 8), None, GAE) + _each((9, 10), 0, GAE) + _each((9, 10), -1, GAE)),
    "kp1_gae_scan_replicas": ([0, P, P, P, P, P, 4, P, P, 4, 8, None],
                              _each((1, 2, 3, 4, 5, 7, 8), None, GAE_R) + _each((9, 10), 0, GAE_R) + _each((9, 10), -1, GAE_R)
                              + [("n_per_replica=0", {6: 0}, GAE_R_N), ("n_per_replica=-4", {6: -4}, GAE_R_N), ("N=8,n_per_replica=3", {6: 3}, GAE_R_N),
                                 ("order:NULL,n_per_replica=3", {1: None, 6: 3}, GAE_R), ("order:T=0,n_per_replica=0", {9: 0, 6: 0}, GAE_R)]),
    "kp1_random_permutation": ([0, 100, P, P, None],
                               _each((2, 3), None, PERM) + _each((1,), 0, PERM) + _each((1,), -1, PERM) + _each((1,), 2**31 + 1, PERM)),
    "kp1_adv_minibatch_stats": ([0, P, 3, P, None], _each((1, 3), None, STATS) + _each((2,), 0, STATS) + _each((2,), -1, STATS)),
    "kp1_adv_minibatch_sums": ([0, P, P, 100, 10, P, None], _each((1, 5), None, SUMS) + _each((3, 4), 0, SUMS) + _each((3, 4), -1, SUMS)),
    "kp1_bootstrap_truncated": ([0, P, P, P, 0.99, 100, None], _each((1, 2, 3), None, BOOT) + _each((5,), 0, BOOT) + _each((5,), -1, BOOT)),
    "kp1_curriculum_create": ([0, 0.8, 10, 5, 3, 0, OUT], [("out_dev=None", {6: None}, NULL)]),
    "kp1_curriculum_create_population": ([0, 2, 0.8, 10, 5, 3, P, OUT],
                                         _each((6, 7), None, NULL) + _each((1,), 0, REPLICAS) + _each((1,), -1, REPLICAS)
                                         + _each((1,), MAX_REPLICAS + 1, REPLICAS)
                                         + [("order:NULL,n_replicas=0", {7: None, 1: 0}, NULL), ("order:NULL,n_replicas=MAX+1", {6: None, 1: MAX_REPLICAS + 1}, NULL)]),
    "kp1_curriculum_observe": ([0, P, P, 64, 1, None], _each((1, 2), None, OBS) + _each((3,), 0, OBS) + _each((3,), -1, OBS)),
    "kp1_curriculum_observe_chunk": ([0, P, P, 64, 2, 2, None], _each((1, 2), None, CHUNK) + _each((3, 4, 5), 0, CHUNK) + _each((3, 4, 5), -1, CHUNK)),
    "kp1_curriculum_observe_population": ([0, P, P, 64, 2, 1, None],
                                          _each((1, 2), None, POP) + _each((3, 4), 0, POP) + _each((3,), -1, POP) + _each((4,), MAX_REPLICAS + 1, POP)),
    "kp1_curriculum_read": ([0, P, P, None], _each((1, 2), None, NULL)),
    "kp1_curriculum_read_replica": ([0, P, 4, 1, P, None],
                                    _each((1, 4), None, NULL) + _each((3,), -1, REPLICA) + _each((3,), 4, REPLICA) + _each((3,), 5, REPLICA)
                                    + [("order:NULL,k=n_replicas", {4: None, 3: 4}, NULL)]),
    "kp1_monitor_create": ([0, 2, 8, 100, 64, OUT],
                           _each((5,), None, M_NULL) + _each((1,), 0, M_REPLICAS) + _each((1,), MAX_REPLICAS + 1, M_REPLICAS) + _each((2,), 0, M_PER)
                           + _each((3,), 0, M_WINDOW) + _each((3,), native.MONITOR_MAX_WINDOW + 1, M_WINDOW)
                           + _each((4,), 0, M_STEPS) + _each((4,), native.MONITOR_MAX_STEPS + 1, M_STEPS)
                           + [("kn*max_steps=2^31", {1: 16, 2: 2**15, 4: 2**12}, M_TOTAL), ("kn*max_steps>2^31", {1: 16, 2: 2**27, 4: 2**12}, M_TOTAL),
                              ("order:NULL,n_replicas=0", {5: None, 1: 0}, M_NULL), ("order:n_replicas=0,n_per_replica=0", {1: 0, 2: 0}, M_REPLICAS),
                              ("order:n_per_replica=0,window=0", {2: 0, 3: 0}, M_PER), ("order:window=0,max_steps=0", {3: 0, 4: 0}, M_WINDOW),
                              ("order:max_steps=MAX+1,kn*max_steps>2^31", {1: 16, 2: 2**20, 4: native.MONITOR_MAX_STEPS + 1}, M_STEPS)]),
    "kp1_monitor_destroy": ([P], [("mon=None", {0: None}, "kp1_monitor_destroy: NULL argument")]),
    # the host buffer as a handle: max_steps = 0 and K = 0, so T = 1 and replica 0 are the first values past the handle's range
    "kp1_monitor_observe": ([P, P, P, 1, None],
                            _each((0, 1, 2), None, MO_NULL) + _each((3,), 0, MO_T) + _each((3,), -1, MO_T) + _each((3,), 1, MO_T)
                            + [("order:NULL,T=0", {1: None, 3: 0}, MO_NULL)]),
    "kp1_monitor_reset_carry": ([P, None], [("mon=None", {0: None}, "kp1_monitor_reset_carry: NULL argument")]),
    "kp1_monitor_read": ([P, 0, STATE, None],
                         _each((0, 2), None, MR_NULL) + _each((1,), -1, MR_REPLICA) + _each((1,), 0, MR_REPLICA) + [("order:NULL,replica=-1", {2: None, 1: -1}, MR_NULL)]),
    "kp1_explained_variance": ([0, P, P, 4, 8, 4, P, None],
                               _each((1, 2, 6), None, EV_NULL) + _each((3, 4, 5), 0, EV_SHAPE) + _each((3, 4, 5), -1, EV_SHAPE)
                               + [("n_total=8,n_per_replica=3", {5: 3}, EV_SHAPE), ("T*n_total=2^31", {3: 2**16, 4: 2**15, 5: 1}, EV_TOTAL),
                                  ("order:NULL,T=0", {6: None, 3: 0}, EV_NULL), ("order:n_per_replica=3,T*n_total=2^31", {3: 2**16, 4: 2**15, 5: 3}, EV_SHAPE)]),
}
CASES = [pytest.param(name, good, changes, text, id=f"{name}-{case}") for name, (good, cases) in TABLE.items() for case, changes, text in cases]


@pytest.mark.parametrize("name,good,changes,text", CASES)
def test_refused_before_the_device_is_selected(name, good, changes, text):
    L = native.load()
    args = list(good)
    assert changes
    for i, v in changes.items():
        args[i] = v
    assert getattr(L, name)(*args) == KP1_ERR_INVALID
    assert L.kp1_last_error().decode() == text


def test_every_refusing_entry_point_of_the_unit_is_in_the_table():
    """the entry points of include/kp1_ppo.h that csrc/kp1_ppo.hip defines; kp1_curriculum_destroy checks nothing before the device"""
    unit = {s for s in native.declared_symbols()
            if s.startswith(("kp1_gae_scan", "kp1_random_permutation", "kp1_adv_minibatch_", "kp1_bootstrap_truncated", "kp1_curriculum_", "kp1_monitor_"))
            or s == "kp1_explained_variance"}
    assert unit - {"kp1_curriculum_destroy"} == set(TABLE)
