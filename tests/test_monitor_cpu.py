"""The training monitor without a GPU: the ABI is exported, declared and bound with matching argument lists and the ctypes struct has the
header's layout; TrainLogger's record, table and progress.csv on fabricated states; what is refused on the host (data parallel, a window
out of range); the CLI flags; and, on fakes, where the trainers launch the monitor -- and that a monitor-off PPO never does."""
from __future__ import annotations

import ctypes as C
import io
import math
import re
import types

import numpy as np
import pytest
import torch

import abi
from rl_brain_trainer_amd import monitor as kmon
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import ppo as kppo

SYMBOLS = {"kp1_monitor_create": 6, "kp1_monitor_destroy": 1, "kp1_monitor_observe": 5, "kp1_monitor_reset_carry": 2, "kp1_monitor_read": 4,
           "kp1_explained_variance": 8}
HEADER = abi.header("kp1_ppo.h")


def same_value(a, b) -> bool:
    """equality of two record values with nan == nan and None == None"""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(str(native.LIB_PATH))
    L = native.load()
    for name, n_args in SYMBOLS.items():
        assert hasattr(lib, name), name
        assert name in native.declared_symbols(), name
        params = abi.params(name, "kp1_ppo.h")
        assert len(getattr(L, name).argtypes) == len(params) == n_args, name
        for text, ctype in zip(params, getattr(L, name).argtypes):
            if "kp1_monitor_state" in text:
                assert ctype is C.POINTER(native.MonitorState), text
            elif "**" in text:
                assert ctype is C.POINTER(C.c_void_p), text
            elif "*" in text:
                assert ctype is C.c_void_p, text
            else:
                assert "int32_t" in text and ctype is C.c_int32, text


def test_struct_layout_matches_the_header():
    """kp1_monitor_state rebuilt from the header's text: same size, and every field at the same offset with the same size"""
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(KP1_MONITOR_\w+)\s+(\d+)", HEADER)}
    assert consts["KP1_MONITOR_MAX_WINDOW"] == native.MONITOR_MAX_WINDOW == 1024
    assert consts["KP1_MONITOR_MAX_STEPS"] == native.MONITOR_MAX_STEPS
    body = re.search(r"typedef struct kp1_monitor_state \{(.*?)\} kp1_monitor_state;", HEADER, flags=re.S).group(1)
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "uint8_t": C.c_uint8}
    fields = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        ctype, names = decl.split(None, 1)
        for name in (n.strip() for n in names.split(",")):
            m = re.fullmatch(r"(\w+)\[(\w+)\]", name)
            fields.append((m.group(1), ctypes_of[ctype] * consts[m.group(2)]) if m else (name, ctypes_of[ctype]))

    class FromHeader(C.Structure):
        _fields_ = fields

    assert C.sizeof(FromHeader) == C.sizeof(native.MonitorState) == 16 + 16 + 1024 * (8 + 4 + 1)
    assert [f[0] for f in fields] == [f[0] for f in native.MonitorState._fields_]
    for name, _ in fields:
        a, b = getattr(FromHeader, name), getattr(native.MonitorState, name)
        assert (a.offset, a.size) == (b.offset, b.size), name


# ---------------------------------------------------------------------------------------------------------------- TrainLogger
def _state(window: int, entries: list[tuple[float, int, int]], *, head: int = 0, total: int | None = None) -> native.MonitorState:
    """a fabricated state whose ring holds `entries` oldest -> newest, starting at slot `head`"""
    st = native.MonitorState()
    st.window, st.ring_len, st.ring_head = window, len(entries), head
    for j, (ret, length, success) in enumerate(entries):
        slot = (head + j) % window
        st.ring_return[slot], st.ring_length[slot], st.ring_success[slot] = ret, length, success
    st.total_episodes = len(entries) if total is None else total
    st.total_successes = sum(e[2] for e in entries)
    return st


def test_returns_are_rounded_to_six_decimals_before_the_mean():
    entries = [(0.1234564, 3, 0), (0.1234566, 5, 1), (2.00000049, 4, 0)]
    rec = kmon.episode_record(_state(8, entries))
    assert rec["rollout/ep_rew_mean"] == float(np.mean([0.123456, 0.123457, 2.0]))
    assert rec["rollout/ep_rew_mean"] != float(np.mean([e[0] for e in entries]))
    assert rec["rollout/ep_len_mean"] == 4.0 and rec["rollout/success_rate"] == 1.0 / 3.0 and rec["rollout/episodes"] == 3


def test_the_ring_is_read_oldest_to_newest_from_ring_head():
    entries = [(float(j) + 0.5, 10 + j, j % 2) for j in range(4)]
    st = _state(4, entries, head=3, total=11)            # a wrapped ring: slot 3 is the oldest, slots 0..2 follow
    assert [st.ring_return[i] for i in range(4)] == [1.5, 2.5, 3.5, 0.5]
    rets, lens, succ = kmon.ring_entries(st)
    assert rets == [0.5, 1.5, 2.5, 3.5] and lens == [10, 11, 12, 13] and succ == [0, 1, 0, 1]
    # the order decides the last bits of a float mean: the record sums oldest -> newest like SB3's deque
    big = [(1e16, 1, 0), (1.0, 1, 0), (-1e16, 1, 0), (1.0, 1, 0)]
    assert kmon.episode_record(_state(4, big, head=2))["rollout/ep_rew_mean"] == float(np.mean([1e16, 1.0, -1e16, 1.0]))
    assert kmon.episode_record(_state(4, entries, head=3, total=11))["rollout/episodes"] == 11


def test_episode_cells_are_empty_before_the_first_episode(tmp_path):
    rec = kmon.episode_record(_state(100, []))
    assert rec == {"rollout/episodes": 0, "rollout/ep_len_mean": None, "rollout/ep_rew_mean": None, "rollout/success_rate": None}
    out = io.StringIO()
    logger = kmon.TrainLogger(tmp_path / "progress.csv", out=out)
    row = logger.log({**rec, "train/explained_variance": kmon.explained_variance(0.0, 1.0), "train/std": 1.0}, iteration=1, total_timesteps=1024)
    header, line = (tmp_path / "progress.csv").read_text().splitlines()
    assert header.split(",") == list(kmon.KEYS)
    cells = dict(zip(header.split(","), line.split(",")))
    assert all(cells[k] == "" for k in kmon.EPISODE_KEYS) and cells["rollout/episodes"] == "0"
    assert cells["train/explained_variance"] == "nan" and math.isnan(row["train/explained_variance"])
    assert "ep_rew_mean" not in out.getvalue() and "episodes" in out.getvalue()     # the table leaves a key without a value out, like SB3
    parsed = kmon.parse_csv_row(header, line)
    assert all(same_value(parsed[k], row[k]) for k in kmon.KEYS)


def test_explained_variance_is_sb3s():
    assert math.isnan(kmon.explained_variance(0.0, 0.0)) and math.isnan(kmon.explained_variance(0.0, 2.0))
    assert kmon.explained_variance(4.0, 1.0) == 0.75 and kmon.explained_variance(1.0, 3.0) == -2.0


def test_csv_and_table_shapes(tmp_path):
    stats = {**kmon.episode_record(_state(100, [(1.25, 20, 1), (-0.5, 30, 0)])), "train/approx_kl": 0.0123456, "train/clip_range": 0.2,
             "train/entropy_loss": -9.93, "train/explained_variance": 0.31, "train/learning_rate": 3e-4, "train/n_updates": 20,
             "train/policy_gradient_loss": -0.004, "train/std": 0.98, "train/value_loss": 12.5, "not/a_key": 1}
    out = io.StringIO()
    logger = kmon.TrainLogger(tmp_path / "sub" / "progress.csv", out=out, start_timesteps=1000)
    rows = [logger.log(stats, iteration=it, total_timesteps=1000 + 2048 * it) for it in (1, 2, 3)]
    assert list(rows[0]) == list(kmon.KEYS) and sorted(kmon.KEYS) == list(kmon.KEYS)
    assert set(kmon.OWN_KEYS) <= set(kmon.KEYS)
    lines = (tmp_path / "sub" / "progress.csv").read_text().splitlines()
    assert len(lines) == 4 and lines[0].split(",") == list(kmon.KEYS)              # one header, one row per logged iteration
    for it, line in zip((1, 2, 3), lines[1:]):
        parsed = kmon.parse_csv_row(lines[0], line)
        assert parsed == rows[it - 1]
        assert parsed["time/iterations"] == it and parsed["time/total_timesteps"] == 1000 + 2048 * it
        assert isinstance(parsed["time/fps"], int) and parsed["time/fps"] > 0 and isinstance(parsed["time/time_elapsed"], int)
        assert parsed["rollout/ep_rew_mean"] == 0.375 and parsed["train/learning_rate"] == 3e-4
    table = out.getvalue().splitlines()[:len(out.getvalue().splitlines()) // 3]
    assert table[0] == table[-1] and set(table[0]) == {"-"}
    assert all(len(line) == len(table[0]) and line.startswith("| ") and line.endswith(" |") for line in table[1:-1])
    names = [line.split("|")[1].rstrip() for line in table[1:-1]]
    assert names[0] == " rollout/" and "    ep_len_mean" in names and " time/" in names and " train/" in names and "    std" in names
    assert names.index(" rollout/") < names.index(" time/") < names.index(" train/")
    values = {line.split("|")[1].strip(): line.split("|")[2].strip() for line in table[1:-1]}
    assert values["ep_len_mean"] == "25" and values["approx_kl"] == "0.0123" and values["n_updates"] == "20" and values["rollout/"] == ""


# ---------------------------------------------------------------------------------------------------------------- host refusals, flags
def test_the_monitor_argument():
    assert kmon.window_of(False) == 0 and kmon.window_of(None) == 0
    assert kmon.window_of(True) == kmon.DEFAULT_WINDOW == 100 and kmon.window_of(37) == 37
    for bad in (0, -1, native.MONITOR_MAX_WINDOW + 1):
        with pytest.raises(ValueError, match="window"):
            kmon.window_of(bad)
    with pytest.raises(TypeError):
        kmon.window_of("yes")


def test_data_parallel_with_the_monitor_is_refused_before_any_device_work(monkeypatch):
    enabled = types.SimpleNamespace(enabled=True, world_size=2, rank=0)
    env = types.SimpleNamespace(dtype=torch.float32)                 # touching anything else of it would raise

    def no_device_work(self, *a, **k):
        raise AssertionError("PPO._setup ran")

    monkeypatch.setattr(kppo.PPO, "_setup", no_device_work)
    for monitor in (True, 50):
        with pytest.raises(ValueError, match="data-parallel"):
            kppo.PPO(env, kppo.PPOConfig(), dist=enabled, monitor=monitor)
    with pytest.raises(AssertionError, match="_setup ran"):          # monitor off: the refusal is not in the way
        kppo.PPO(env, kppo.PPOConfig(), dist=enabled, monitor=False)
    assert kmon.check_monitor(True, types.SimpleNamespace(enabled=False)) == 100
    assert kmon.check_monitor(False, enabled) == 0


@pytest.mark.parametrize("module", ["train", "train_dock", "train_route"])
def test_cli_flags(module):
    import importlib

    parser = importlib.import_module(f"rl_brain_trainer_amd.{module}").build_arg_parser()
    required = {"train": ["--config", "c.yaml"], "train_dock": ["--config", "c.yaml"], "train_route": ["--config", "c.yaml"]}[module]
    off = parser.parse_args(required)
    assert off.monitor is False and off.stats_window_size == 100 and kmon.cli_monitor(off) is False
    assert kmon.check_monitor(kmon.cli_monitor(off), types.SimpleNamespace(enabled=True)) == 0      # what the trainers get without the flag is "off"
    on = parser.parse_args(required + ["--monitor"])
    assert kmon.cli_monitor(on) == 100
    sized = parser.parse_args(required + ["--monitor", "--stats-window-size", "20"])
    assert kmon.cli_monitor(sized) == 20
    assert kmon.cli_monitor(parser.parse_args(required + ["--stats-window-size", "20"])) is False     # the size alone switches nothing on
    with pytest.raises(ValueError, match="window"):
        kmon.cli_monitor(parser.parse_args(required + ["--monitor", "--stats-window-size", "0"]))


# ---------------------------------------------------------------------------------------------------------------- launch placement on fakes
class _FakeLib:
    def __init__(self, log: list) -> None:
        self.log = log

    def kp1_gae_scan(self, *a):
        self.log.append("gae")
        return 0

    def kp1_explained_variance(self, dev, values, returns, T, n_total, n_per_replica, out, stream):
        self.log.append(("explained_variance", T, n_total, n_per_replica))
        return 0

    def __getattr__(self, name):
        raise AssertionError(f"unexpected library call {name}")


class _FakeMonitor:
    def __init__(self, log: list) -> None:
        self.log = log

    def observe(self, rewards, dones, T):
        self.log.append(("observe", T, tuple(rewards.shape), float(rewards.sum())))

    def reset_carry(self):
        self.log.append("reset_carry")


def _fake_ppo(log: list, monitor: bool, monkeypatch, K: int = 1):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    p = object.__new__(kppo.PPO)
    T, N = 4, 3
    p.cfg = kppo.PPOConfig(n_steps=T, batch_size=4, hidden=64)
    p.K, p.n_envs, p.device, p.obs_w = K, N, torch.device("cpu"), 64
    p.L = _FakeLib(log)
    for name in ("rew_buf", "val_buf", "adv_buf", "ret_buf"):
        setattr(p, name, torch.zeros((T, K * N)))
    p.done_buf = torch.zeros((T, K * N), dtype=torch.uint8)
    p.obs_buf = torch.zeros((T + 1, K * N, 64))
    p._mlp = types.SimpleNamespace(forward=lambda obs, value=None: log.append("last value"))

    def bootstrap() -> None:
        log.append("bootstrap")
        p.rew_buf += 1.0                     # the mutation the monitor must not see

    p._bootstrap_truncated = bootstrap
    p.envs = [types.SimpleNamespace(reset=lambda: torch.zeros((N, 64)))]
    if monitor:
        p.monitor = _FakeMonitor(log)
        p._ev_dev = torch.zeros((K, 2), dtype=torch.float64)
    return p


def test_a_monitor_off_ppo_makes_no_monitor_call(monkeypatch):
    log: list = []
    p = _fake_ppo(log, False, monkeypatch)
    assert p.monitor is None
    p._post_rollout()
    p._reset_envs()
    assert log == ["bootstrap", "last value", "gae"]                 # the tail as it was: any monitor entry point would have raised or logged


def test_the_monitor_launches_first_and_the_explained_variance_last(monkeypatch):
    log: list = []
    p = _fake_ppo(log, True, monkeypatch)
    p._post_rollout()
    assert log == [("observe", 4, (4, 3), 0.0), "bootstrap", "last value", "gae", ("explained_variance", 4, 3, 3)]
    log.clear()
    p._reset_envs()
    assert log == ["reset_carry"]
    log.clear()
    p._monitor_live = False                                          # the capture warm-up's tail: its one step is no episode data
    p._post_rollout()
    assert log == ["bootstrap", "last value", "gae", ("explained_variance", 4, 3, 3)]


def test_population_tail_with_overrides_has_the_same_placement(monkeypatch):
    from rl_brain_trainer_amd import population as kpop

    log: list = []
    p = _fake_ppo(log, True, monkeypatch, K=2)
    p.__class__ = kpop.PopulationPPO
    p.has_overrides = True
    p._gamma_lambda = torch.zeros((2, 2))
    p.L.kp1_gae_scan_replicas = lambda *a: (log.append("gae replicas"), 0)[1]
    p._post_rollout()
    assert log == [("observe", 4, (4, 6), 0.0), "bootstrap", "last value", "gae replicas", ("explained_variance", 4, 6, 3)]
