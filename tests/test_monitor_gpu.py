"""Training monitor on the GPU (include/kp1_ppo.h kp1_monitor_*, kp1_explained_variance; rl_brain_trainer_amd/monitor.py).

The kernel cases run on synthetic buffers and are compared, byte for byte, with a restatement of SB3's Monitor.step +
OnPolicyAlgorithm._update_info_buffer: a Python loop with one fp64 carry per env and a collections.deque(maxlen=window) per replica.
The trainer cases check that the monitor sees the rewards before the time-limit bootstrap, that graphs / the whole-rollout launch / a
population leave the same states, and that switching it on perturbs nothing of the training itself."""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import monitor as kmon
from rl_brain_trainer_amd import native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
END = native.DONE_TERMINATED | native.DONE_TRUNCATED


def same_value(a, b) -> bool:
    """equality of two record values with nan == nan and None == None"""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b


# ---------------------------------------------------------------------------------------------------------------- the restatement
class RefMonitor:
    """Monitor.step per env (rewards summed as Python floats = fp64, in step order; a length count) and ep_info_buffer per replica"""

    def __init__(self, K: int, N: int, window: int) -> None:
        self.K, self.N, self.window = K, N, window
        self.ret = [0.0] * (K * N)
        self.len = [0] * (K * N)
        self.rings = [collections.deque(maxlen=window) for _ in range(K)]
        self.heads = [0] * K          # slot of the oldest entry: 0 while the ring fills, then one further per episode
        self.episodes = [0] * K
        self.successes = [0] * K

    def reset_carry(self) -> None:
        self.ret = [0.0] * (self.K * self.N)
        self.len = [0] * (self.K * self.N)

    def observe(self, rewards: np.ndarray, dones: np.ndarray) -> None:
        T = rewards.shape[0]
        for t in range(T):
            for k in range(self.K):          # (t, then env index) order inside every replica
                for n in range(self.N):
                    i = k * self.N + n
                    self.ret[i] += float(rewards[t, i])
                    self.len[i] += 1
                    d = int(dones[t, i])
                    if d & END:
                        if len(self.rings[k]) == self.window:
                            self.heads[k] = (self.heads[k] + 1) % self.window
                        self.rings[k].append((self.ret[i], self.len[i], 1 if d & native.DONE_SUCCESS else 0))
                        self.episodes[k] += 1
                        self.successes[k] += 1 if d & native.DONE_SUCCESS else 0
                        self.ret[i], self.len[i] = 0.0, 0


def _state_bytes(st) -> bytes:
    return bytes(C.string_at(C.addressof(st), C.sizeof(st)))


def _assert_matches(mon: kmon.EpisodeMonitor, ref: RefMonitor, what) -> None:
    for k in range(ref.K):
        st = mon.read(k)
        rets, lens, succ = kmon.ring_entries(st)
        want = list(ref.rings[k])
        assert st.window == ref.window, (what, k)
        assert st.ring_len == len(want), (what, k, st.ring_len, len(want))
        assert st.ring_head == ref.heads[k], (what, k, st.ring_head, ref.heads[k])
        assert np.array(rets, dtype=np.float64).tobytes() == np.array([w[0] for w in want], dtype=np.float64).tobytes(), (what, k, "returns")
        assert lens == [w[1] for w in want], (what, k, "lengths")
        assert succ == [w[2] for w in want], (what, k, "success bytes")
        assert st.total_episodes == ref.episodes[k] and st.total_successes == ref.successes[k], (what, k, "totals")


def _draw(g: np.random.Generator, T: int, KN: int, p_end: float = 0.15) -> tuple[np.ndarray, np.ndarray]:
    """seeded fp32 rewards; done bytes from {0, 1, 2, 5, 6, 4}: an end with probability p_end, else 0 or (one time in ten) the bare
    success bit 4, which ends nothing"""
    rewards = (g.standard_normal((T, KN)) * 3.0 + 0.25).astype(np.float32)
    u = g.random((T, KN))
    ends = g.choice(np.array([1, 2, 5, 6], dtype=np.uint8), size=(T, KN))
    idle = np.where(g.random((T, KN)) < 0.1, 4, 0).astype(np.uint8)
    return rewards, np.where(u < p_end, ends, idle).astype(np.uint8)


def _feed(mon: kmon.EpisodeMonitor, ref: RefMonitor, rewards: np.ndarray, dones: np.ndarray) -> None:
    mon.observe(torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV))
    ref.observe(rewards, dones)


def _closing_call(g: np.random.Generator, KN: int) -> tuple[np.ndarray, np.ndarray]:
    """one step in which every env ends: exposes every carry (return and length) as an episode"""
    rewards = g.standard_normal((1, KN)).astype(np.float32)
    return rewards, np.full((1, KN), 2, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- kernels vs restatement
@pytest.mark.parametrize("window", [8, 100])
@pytest.mark.parametrize("K,N,T", [(1, 1, 24), (1, 33, 24), (1, 70, 24), (3, 16, 24), (1, 33, 1), (3, 16, 1)])
def test_random_draws_match_the_restatement(K, N, T, window):
    g = np.random.default_rng(1000 * K + 10 * N + T + window)
    mon, ref = kmon.EpisodeMonitor(DEV, K, N, window=window, max_steps=24), RefMonitor(K, N, window)
    for call in range(3):                                  # the later calls run on the earlier calls' carries and rings
        _feed(mon, ref, *_draw(g, T, K * N))
        _assert_matches(mon, ref, ("call", call))
    _feed(mon, ref, *_closing_call(g, K * N))
    _assert_matches(mon, ref, "carries")
    if (K, N, T, window) == (1, 70, 24, 100):
        assert ref.episodes[0] > 100 and ref.heads[0] != 0, "N = 70 was meant to overflow window 100 (the ring wraps)"
    if (K, N, T, window) == (1, 1, 24, 100):
        assert ref.episodes[0] < 100 and ref.heads[0] == 0, "N = 1 was meant to stay below window 100"
    mon.close()


def test_a_buffer_without_any_end_moves_only_the_carries():
    K, N, T, window = 3, 16, 24, 8
    g = np.random.default_rng(5)
    mon, ref = kmon.EpisodeMonitor(DEV, K, N, window=window, max_steps=T), RefMonitor(K, N, window)
    _feed(mon, ref, *_draw(g, T, K * N))
    before = [_state_bytes(mon.read(k)) for k in range(K)]
    rewards, dones = _draw(g, T, K * N, p_end=0.0)
    assert not (dones & END).any() and (dones == 4).any()
    _feed(mon, ref, rewards, dones)
    assert [_state_bytes(mon.read(k)) for k in range(K)] == before
    _feed(mon, ref, *_closing_call(g, K * N))              # the carries advanced by T steps and their rewards
    _assert_matches(mon, ref, "carries")
    assert all(w[1] >= T + 1 for w in ref.rings[0])
    mon.close()


def _built(T: int, KN: int, ends: list[tuple[int, int, int]], seed: int) -> tuple[np.ndarray, np.ndarray]:
    g = np.random.default_rng(seed)
    rewards = g.standard_normal((T, KN)).astype(np.float32)
    dones = np.zeros((T, KN), dtype=np.uint8)
    for t, i, byte in ends:
        dones[t, i] = byte
    return rewards, dones


@pytest.mark.parametrize("extra", [0, 1])
def test_exactly_window_and_window_plus_one_episodes_in_one_call(extra):
    K, N, T, window = 1, 3, 4, 8
    cells = [(t, i) for t in range(T) for i in range(N)][:window + extra]
    rewards, dones = _built(T, N, [(t, i, (1, 2, 5, 6)[(t + i) % 4]) for t, i in cells], seed=extra)
    mon, ref = kmon.EpisodeMonitor(DEV, K, N, window=window, max_steps=T), RefMonitor(K, N, window)
    _feed(mon, ref, rewards, dones)
    assert ref.episodes[0] == window + extra and ref.heads[0] == extra
    _assert_matches(mon, ref, "built")
    _feed(mon, ref, *_closing_call(np.random.default_rng(9), N))
    _assert_matches(mon, ref, "carries")
    mon.close()


def test_ends_at_the_first_and_the_last_step_and_around_the_wave_boundary():
    K, N, T, window = 1, 70, 24, 100
    ends = [(0, 0, 1), (0, 69, 6), (T - 1, 5, 2), (T - 1, 64, 5)]
    ends += [(11, i, (2, 5, 1, 6)[i % 4]) for i in (61, 62, 63, 64, 65, 66)]       # several ends of one row on both sides of lane 63 / 64
    rewards, dones = _built(T, N, ends, seed=3)
    dones[4, 10] = 4                                                                 # a bare success bit: no end
    mon, ref = kmon.EpisodeMonitor(DEV, K, N, window=window, max_steps=T), RefMonitor(K, N, window)
    _feed(mon, ref, rewards, dones)
    assert ref.episodes[0] == len(ends)
    # t = 0 ends after one step; env 5 runs the whole call, env 64 ended in row 11 and again in the last row
    assert [w[1] for w in ref.rings[0]][:2] == [1, 1] and [w[1] for w in ref.rings[0]][-2:] == [T, T - 12]
    _assert_matches(mon, ref, "built")
    _feed(mon, ref, *_closing_call(np.random.default_rng(4), N))
    _assert_matches(mon, ref, "carries")
    mon.close()


@pytest.mark.parametrize("K,N,window", [(3, 16, 8), (1, 70, 100)])
def test_a_split_call_leaves_the_bytes_of_one_call(K, N, window):
    T, a = 24, 7
    g = np.random.default_rng(77 + N)
    whole = kmon.EpisodeMonitor(DEV, K, N, window=window, max_steps=T)
    split = kmon.EpisodeMonitor(DEV, K, N, window=window, max_steps=T)
    ref = RefMonitor(K, N, window)
    for _ in range(2):
        rewards, dones = _draw(g, T, K * N)
        r_dev, d_dev = torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV)
        whole.observe(r_dev, d_dev)
        split.observe(r_dev[:a], d_dev[:a])
        split.observe(r_dev[a:], d_dev[a:])
        ref.observe(rewards, dones)
        assert [_state_bytes(whole.read(k)) for k in range(K)] == [_state_bytes(split.read(k)) for k in range(K)]
        _assert_matches(split, ref, "split")
    rewards, dones = _closing_call(g, K * N)
    for mon in (whole, split):
        mon.observe(torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV))
    ref.observe(rewards, dones)
    assert [_state_bytes(whole.read(k)) for k in range(K)] == [_state_bytes(split.read(k)) for k in range(K)]
    _assert_matches(split, ref, "carries")
    whole.close()
    split.close()


def test_reset_carry_between_two_calls():
    K, N, T, window = 3, 16, 24, 100
    g = np.random.default_rng(21)
    mon, ref = kmon.EpisodeMonitor(DEV, K, N, window=window, max_steps=T), RefMonitor(K, N, window)
    _feed(mon, ref, *_draw(g, T, K * N))
    before = [_state_bytes(mon.read(k)) for k in range(K)]
    mon.reset_carry()
    ref.reset_carry()
    assert [_state_bytes(mon.read(k)) for k in range(K)] == before          # rings and totals stay
    _feed(mon, ref, *_closing_call(g, K * N))
    assert all(w[1] == 1 for w in list(ref.rings[0])[-N:])
    _assert_matches(mon, ref, "after reset_carry")
    mon.close()


def test_refusals_leave_the_handle_untouched():
    L = native.load()
    K, N, T, window = 2, 16, 24, 8
    g = np.random.default_rng(2)
    mon, ref = kmon.EpisodeMonitor(DEV, K, N, window=window, max_steps=T), RefMonitor(K, N, window)
    _feed(mon, ref, *_draw(g, T, K * N))
    before = [_state_bytes(mon.read(k)) for k in range(K)]
    r = torch.zeros((T, K * N), dtype=torch.float32, device=DEV)
    d = torch.full((T, K * N), 2, dtype=torch.uint8, device=DEV)
    rp, dp, h = C.c_void_p(r.data_ptr()), C.c_void_p(d.data_ptr()), mon._h
    out = native.MonitorState()

    def refused(rc: int, text: str) -> None:
        assert rc == -1 and text in L.kp1_last_error().decode(), (rc, L.kp1_last_error())

    refused(L.kp1_monitor_observe(None, rp, dp, T, None), "NULL")
    refused(L.kp1_monitor_observe(h, None, dp, T, None), "NULL")
    refused(L.kp1_monitor_observe(h, rp, None, T, None), "NULL")
    refused(L.kp1_monitor_observe(h, rp, dp, 0, None), "T must be in")
    refused(L.kp1_monitor_observe(h, rp, dp, -3, None), "T must be in")
    refused(L.kp1_monitor_observe(h, rp, dp, T + 1, None), "T must be in")
    refused(L.kp1_monitor_read(h, -1, C.byref(out), None), "replica index out of range")
    refused(L.kp1_monitor_read(h, K, C.byref(out), None), "replica index out of range")
    refused(L.kp1_monitor_read(h, 0, None, None), "NULL")
    refused(L.kp1_monitor_read(None, 0, C.byref(out), None), "NULL")
    refused(L.kp1_monitor_reset_carry(None, None), "NULL")
    refused(L.kp1_monitor_destroy(None), "NULL")
    made = C.c_void_p()
    refused(L.kp1_monitor_create(0, K, N, window, T, None), "NULL")
    refused(L.kp1_monitor_create(0, K, N, 0, T, C.byref(made)), "window must be in")
    refused(L.kp1_monitor_create(0, K, N, native.MONITOR_MAX_WINDOW + 1, T, C.byref(made)), "window must be in")
    refused(L.kp1_monitor_create(0, 0, N, window, T, C.byref(made)), "n_replicas must be in")
    refused(L.kp1_monitor_create(0, 17, N, window, T, C.byref(made)), "n_replicas must be in")
    refused(L.kp1_monitor_create(0, K, 0, window, T, C.byref(made)), "n_per_replica")
    refused(L.kp1_monitor_create(0, K, N, window, 0, C.byref(made)), "max_steps must be in")
    refused(L.kp1_monitor_create(0, K, N, window, native.MONITOR_MAX_STEPS + 1, C.byref(made)), "max_steps must be in")
    assert not made.value
    ev = torch.zeros((K, 2), dtype=torch.float64, device=DEV)
    refused(L.kp1_explained_variance(0, None, rp, T, K * N, N, C.c_void_p(ev.data_ptr()), None), "NULL")
    refused(L.kp1_explained_variance(0, rp, rp, T, K * N, N, None, None), "NULL")
    refused(L.kp1_explained_variance(0, rp, rp, 0, K * N, N, C.c_void_p(ev.data_ptr()), None), "multiple of n_per_replica")
    refused(L.kp1_explained_variance(0, rp, rp, T, K * N, N + 1, C.c_void_p(ev.data_ptr()), None), "multiple of n_per_replica")
    with pytest.raises(ValueError):
        mon.observe(r, d, T + 1)
    torch.cuda.synchronize()
    assert [_state_bytes(mon.read(k)) for k in range(K)] == before
    _feed(mon, ref, *_closing_call(g, K * N))              # the carries were not touched either
    _assert_matches(mon, ref, "after the refusals")
    mon.close()


# ---------------------------------------------------------------------------------------------------------------- explained variance
def _explained_variance_dev(values: np.ndarray, returns: np.ndarray, N: int) -> list[float]:
    L = native.load()
    T, KN = values.shape
    v, y = torch.from_numpy(values).to(DEV), torch.from_numpy(returns).to(DEV)
    out = torch.zeros((KN // N, 2), dtype=torch.float64, device=DEV)
    native.check(L.kp1_explained_variance(0, C.c_void_p(v.data_ptr()), C.c_void_p(y.data_ptr()), T, KN, N, C.c_void_p(out.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    return [kmon.explained_variance(a, b) for a, b in out.tolist()]


@pytest.mark.parametrize("K,N,T", [(1, 128, 64), (3, 33, 64), (1, 1, 5)])
def test_explained_variance_matches_numpy_two_pass_fp64(K, N, T):
    """numpy's np.var is two-pass; inputs are the same fp32 numbers widened to fp64.  Tolerance 1e-8 absolute on the explained variance: a
    sum of n <= 8192 fp64 terms is off by at most n 2^-53 = 9e-13 relative, the single-pass form amplifies that by at most
    1 + 2 mean^2 / var <= 201 under |mean| <= 10 std, i.e. about 2e-10: a 40-fold margin."""
    assert T * N <= 8192
    g = np.random.default_rng(31 * K + N)
    means = g.uniform(-8.0, 8.0, size=K)
    returns = np.concatenate([(g.standard_normal((T, N)) + means[k]) for k in range(K)], axis=1).astype(np.float32)
    values = (returns * 0.7 + g.standard_normal((T, K * N)) * 0.5 + 0.3).astype(np.float32)
    got = _explained_variance_dev(values, returns, N)
    for k in range(K):
        y, v = returns[:, k * N:(k + 1) * N].astype(np.float64), values[:, k * N:(k + 1) * N].astype(np.float64)
        assert abs(y.mean()) <= 10.0 * y.std() and abs((y - v).mean()) <= 10.0 * (y - v).std()
        want = 1.0 - np.var(y - v) / np.var(y)
        assert abs(got[k] - want) <= 1e-8, (k, got[k], want)


def test_explained_variance_of_constant_returns_is_nan():
    T, N, K = 64, 33, 2
    g = np.random.default_rng(8)
    returns = np.full((T, K * N), 3.1415927, dtype=np.float32)
    returns[:, N:] = g.standard_normal((T, N)).astype(np.float32)
    values = g.standard_normal((T, K * N)).astype(np.float32)
    got = _explained_variance_dev(values, returns, N)
    assert math.isnan(got[0]) and math.isfinite(got[1])


# ---------------------------------------------------------------------------------------------------------------- trainers
def _env_cfg():
    return kcfg.to_env_config(kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"))


N_ENVS, N_STEPS, ITERATIONS = 16, 64, 2


def _pcfg(seed: int = 7):
    from rl_brain_trainer_amd.ppo import PPOConfig

    return PPOConfig(n_steps=N_STEPS, batch_size=256, n_epochs=2, hidden=64, learning_rate=3e-4, ent_coef=1e-3, seed=seed)


def _run_single(env_cfg, *, monitor, use_graphs: bool, seed: int = 7, snapshots: list | None = None):
    from rl_brain_trainer_amd.ppo import PPO
    from rl_brain_trainer_amd.vec_env import ArmKinematicVecEnv

    ppo = PPO(ArmKinematicVecEnv(env_cfg, N_ENVS, seed=seed), _pcfg(seed), use_graphs=use_graphs, monitor=monitor)
    if snapshots is not None:
        bootstrap = ppo._bootstrap_truncated

        def spy() -> None:
            before = ppo.rew_buf.clone()                                       # what the env wrote, before gamma * V is added
            bootstrap()
            snapshots.append((before, ppo.done_buf.clone(), ppo.rew_buf.clone()))

        ppo._bootstrap_truncated = spy
    for _ in range(ITERATIONS):
        ppo.collect_rollouts()
        ppo.train()
    torch.cuda.synchronize()
    return ppo


@pytest.fixture(scope="module")
def eager_run():
    """the eager monitored run, its pre-bootstrap (rewards, done bytes) of every rollout and the restatement fed with them"""
    env_cfg = _env_cfg()
    snaps: list = []
    ppo = _run_single(env_cfg, monitor=True, use_graphs=False, snapshots=snaps)
    assert len(snaps) == ITERATIONS
    ref = RefMonitor(1, N_ENVS, kmon.DEFAULT_WINDOW)
    for rew, done, _after in snaps:
        ref.observe(rew.cpu().numpy(), done.cpu().numpy())
    states = [_state_bytes(ppo.monitor.read(0))]
    out = {"env_cfg": env_cfg, "snaps": snaps, "ref": ref, "states": states, "rows": ppo.monitor_rows()}
    ppo.env.close()
    return out


def test_the_monitor_sees_the_rewards_before_the_bootstrap(eager_run):
    snaps, ref = eager_run["snaps"], eager_run["ref"]
    assert any(bool(((d & 3) == 2).any()) for _, d, _ in snaps), "no truncated step: the before / after distinction carries no weight"
    assert any(not torch.equal(before, after) for before, _, after in snaps), "the bootstrap changed no reward"
    assert ref.episodes[0] > 0
    mon_state = eager_run["states"][0]
    st = native.MonitorState.from_buffer_copy(mon_state)
    rets, lens, succ = kmon.ring_entries(st)
    want = list(ref.rings[0])
    assert st.ring_len == len(want) and st.ring_head == ref.heads[0]
    assert np.array(rets, dtype=np.float64).tobytes() == np.array([w[0] for w in want], dtype=np.float64).tobytes()
    assert lens == [w[1] for w in want] and succ == [w[2] for w in want]
    assert st.total_episodes == ref.episodes[0] and st.total_successes == ref.successes[0]
    row = eager_run["rows"][0]
    assert row["rollout/episodes"] == ref.episodes[0]
    assert row["rollout/ep_rew_mean"] == float(np.mean([round(w[0], 6) for w in want]))
    assert row["rollout/ep_len_mean"] == float(np.mean([w[1] for w in want]))
    assert row["train/n_updates"] == ITERATIONS * 2 and 0.5 < row["train/std"] < 2.0
    assert math.isfinite(row["train/explained_variance"]) and row["train/entropy_loss"] < 0


@pytest.mark.parametrize("form", ["graphs", "whole-rollout"])
def test_graphs_and_the_whole_rollout_launch_leave_the_same_states(form, eager_run, monkeypatch):
    if form == "whole-rollout":
        monkeypatch.setenv("KP1_ROLLOUT_RUN", "1")
    else:
        monkeypatch.delenv("KP1_ROLLOUT_RUN", raising=False)
    ppo = _run_single(eager_run["env_cfg"], monitor=True, use_graphs=True)
    assert ppo._rollout_graph is not None and bool(ppo._whole_rollout) == (form == "whole-rollout")
    assert _state_bytes(ppo.monitor.read(0)) == eager_run["states"][0]
    rows = ppo.monitor_rows()
    assert all(same_value(rows[0][k], eager_run["rows"][0][k]) for k in rows[0]), (rows, eager_run["rows"])
    ppo.env.close()


def test_the_monitor_perturbs_nothing(eager_run):
    """a PPO with the monitor on against a twin with it off: parameters, Adam state, last_stats and rollout buffers, bit for bit"""
    on = _run_single(eager_run["env_cfg"], monitor=True, use_graphs=True)
    off = _run_single(eager_run["env_cfg"], monitor=False, use_graphs=True)
    assert off.monitor is None
    with pytest.raises(RuntimeError, match="monitor=True"):
        off.monitor_rows()
    assert torch.equal(on.policy.flat, off.policy.flat)
    assert torch.equal(on.adam_m, off.adam_m) and torch.equal(on.adam_v, off.adam_v) and on.adam_t == off.adam_t
    assert on.last_stats == off.last_stats
    for name in ("rew_buf", "done_buf", "adv_buf", "ret_buf", "val_buf", "obs_buf"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name
    on.env.close()
    off.env.close()


def test_approach_population_replicas_match_single_monitored_runs():
    from rl_brain_trainer_amd.population import ApproachPopulationPPO
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv

    env_cfg, seeds = _env_cfg(), [7, 8]
    penv = ArmKinematicPopulationVecEnv(env_cfg, seeds, N_ENVS)
    pop = ApproachPopulationPPO(seeds, dataclasses.replace(_pcfg()), penv, monitor=True)
    for _ in range(ITERATIONS):
        pop.collect_rollouts()
        pop.train()
    rows = pop.monitor_rows()
    for k, s in enumerate(seeds):
        single = _run_single(env_cfg, monitor=True, use_graphs=True, seed=s)
        assert _state_bytes(single.monitor.read(0)) == _state_bytes(pop.monitor.read(k)), k
        one = single.monitor_rows()[0]
        assert all(same_value(one[key], rows[k][key]) for key in one), (k, one, rows[k])
        single.env.close()
    assert rows[0]["rollout/episodes"] > 0 and _state_bytes(pop.monitor.read(0)) != _state_bytes(pop.monitor.read(1))
    pop.close()
    penv.close()


def test_train_cli_monitor_writes_progress_csv(tmp_path, monkeypatch, capsys):
    import yaml

    from rl_brain_trainer_amd import ppo as kppo
    from rl_brain_trainer_amd import train

    seen: list = []
    real_rows = kppo.PPO.monitor_rows

    def spy(self):
        rows = real_rows(self)
        seen.append(rows)
        return rows

    monkeypatch.setattr(kppo.PPO, "monitor_rows", spy)
    overlay = {"base_config": str(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"),
               "workspace_expansion": {"init_approach_checkpoint": "", "finisher_checkpoint": ""}}
    cfg_path = tmp_path / "run.yaml"
    cfg_path.write_text(yaml.safe_dump(overlay))
    root = tmp_path / "run"
    train.main(["--config", str(cfg_path), "--total-timesteps", str(2 * N_ENVS * N_STEPS), "--n-envs", str(N_ENVS), "--n-steps", str(N_STEPS),
                "--batch-size", "256", "--hidden", "64", "--log-every", "1", "--run-id", "m", "--artifact-root", str(root), "--seed", "7",
                "--monitor", "--stats-window-size", "50"])
    lines = (root / "progress.csv").read_text().splitlines()
    assert lines[0].split(",") == list(kmon.KEYS)
    assert len(lines) == 1 + ITERATIONS and len(seen) == ITERATIONS
    last = kmon.parse_csv_row(lines[0], lines[-1])
    assert last["time/iterations"] == ITERATIONS and last["time/total_timesteps"] == ITERATIONS * N_ENVS * N_STEPS
    assert last["time/fps"] > 0 and last["time/time_elapsed"] >= 0
    for key, value in seen[-1][0].items():
        assert same_value(last[key], value), (key, last[key], value)
    assert last["rollout/episodes"] > 0 and last["train/n_updates"] > 0
    text = capsys.readouterr().out
    assert "| rollout/" in text and "ep_rew_mean" in text and "explained_variance" in text and "[ppo] it=" not in text


def test_train_cli_seeds_writes_one_progress_csv_per_replica(tmp_path, capsys):
    import yaml

    from rl_brain_trainer_amd import train

    overlay = {"base_config": str(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml"),
               "workspace_expansion": {"init_approach_checkpoint": "", "finisher_checkpoint": ""}}
    cfg_path = tmp_path / "run.yaml"
    cfg_path.write_text(yaml.safe_dump(overlay))
    root = tmp_path / "pop"
    train.main(["--config", str(cfg_path), "--total-timesteps", str(2 * N_ENVS * N_STEPS), "--n-envs", str(N_ENVS), "--n-steps", str(N_STEPS),
                "--batch-size", "256", "--hidden", "64", "--log-every", "1", "--run-id", "p", "--artifact-root", str(root), "--seeds", "7,8",
                "--monitor"])
    rows = {}
    for s in (7, 8):
        lines = (root / f"seed_{s}" / "progress.csv").read_text().splitlines()      # next to the replica's model_latest.zip
        assert (root / f"seed_{s}" / "model_latest.zip").is_file()
        assert lines[0].split(",") == list(kmon.KEYS) and len(lines) == 1 + ITERATIONS
        rows[s] = kmon.parse_csv_row(lines[0], lines[-1])
        assert rows[s]["time/iterations"] == ITERATIONS and rows[s]["time/total_timesteps"] == ITERATIONS * N_ENVS * N_STEPS
        assert rows[s]["rollout/episodes"] > 0 and math.isfinite(rows[s]["train/explained_variance"])
    assert rows[7]["rollout/ep_rew_mean"] != rows[8]["rollout/ep_rew_mean"]
    text = capsys.readouterr().out
    assert "replica seed_7" in text and "replica seed_8" in text and text.count("| rollout/") == 2 * ITERATIONS
