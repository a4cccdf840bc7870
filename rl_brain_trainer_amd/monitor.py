"""Training monitor: SB3's per-iteration record of a running training, from statistics kept on the device.

The reference trains through ``make_vec_env`` (every env in a ``Monitor``) with ``PPO(..., verbose=1)``, so its users watch SB3's table:
``rollout/ep_rew_mean`` and ``rollout/ep_len_mean`` over the newest ``stats_window_size`` episodes, ``train/explained_variance``,
``train/std``, the loss terms and ``time/fps``.  Here the rollout is a captured graph, so the episode statistics are taken by kernels in
that graph's tail (include/kp1_ppo.h, kp1_monitor_* and kp1_explained_variance) and read back only when a record is asked for:

* ``EpisodeMonitor`` wraps the device handle: K replicas x N envs, per env a running (return, length), per replica a ring of the newest
  ``window`` episodes and two totals;
* ``TrainLogger`` turns one iteration's numbers into SB3's record, prints SB3's boxed table and appends to ``progress.csv`` in
  ``CSVOutputFormat``'s shape (a header of keys, one row per logged iteration).

Two keys are this engine's own and have no SB3 counterpart of the same meaning in the reference's runs: ``rollout/success_rate`` (share of
successes among the episodes of the ring, from the env's success bit) and ``rollout/episodes`` (episodes ended since the start).
"""
from __future__ import annotations

import ctypes as C
import sys
import time
from pathlib import Path
from typing import Any, TextIO

import numpy as np

from . import native

DEFAULT_WINDOW = 100          # SB3's stats_window_size

# the record, in the order SB3's table sorts it (and the header of progress.csv)
KEYS = (
    "rollout/ep_len_mean", "rollout/ep_rew_mean", "rollout/episodes", "rollout/success_rate",
    "time/fps", "time/iterations", "time/time_elapsed", "time/total_timesteps",
    "train/approx_kl", "train/clip_range", "train/entropy_loss", "train/explained_variance", "train/learning_rate", "train/n_updates",
    "train/policy_gradient_loss", "train/std", "train/value_loss",
)
OWN_KEYS = ("rollout/success_rate", "rollout/episodes")                       # not SB3's
EPISODE_KEYS = ("rollout/ep_len_mean", "rollout/ep_rew_mean", "rollout/success_rate")   # empty until a first episode has ended


def window_of(monitor: Any) -> int:
    """the trainers' ``monitor=`` argument -> ring size: False / None = 0 (off), True = SB3's default of 100, an int = that window"""
    if monitor is None or monitor is False:
        return 0
    if monitor is True:
        return DEFAULT_WINDOW
    if isinstance(monitor, (int, np.integer)):
        w = int(monitor)
        if not 1 <= w <= native.MONITOR_MAX_WINDOW:
            raise ValueError(f"monitor={w}: the episode window must be in [1, {native.MONITOR_MAX_WINDOW}]")
        return w
    raise TypeError(f"monitor must be False, True or a window size, not {monitor!r}")


def check_monitor(monitor: Any, dist: Any) -> int:
    """window_of, and the refusal of a data-parallel run (cross-rank episode order is not defined here): on the host, before any device work"""
    w = window_of(monitor)
    if w and getattr(dist, "enabled", False):
        raise ValueError("the training monitor is single-process: a data-parallel run (torch.distributed) cannot take monitor=")
    return w


def ring_entries(state: native.MonitorState) -> tuple[list[float], list[int], list[int]]:
    """(returns, lengths, successes) of a state's ring, oldest -> newest: ring_len slots from ring_head on"""
    w, n, h = int(state.window), int(state.ring_len), int(state.ring_head)
    order = [(h + j) % w for j in range(n)]
    return [float(state.ring_return[i]) for i in order], [int(state.ring_length[i]) for i in order], [int(state.ring_success[i]) for i in order]


def episode_record(state: native.MonitorState) -> dict[str, Any]:
    """the rollout/ keys of one replica.  Monitor.step rounds an episode's return to 6 decimals before it reports it, and
    OnPolicyAlgorithm's safe_mean averages the deque oldest -> newest; the episode keys are None until a first episode has ended."""
    rets, lens, succ = ring_entries(state)
    out: dict[str, Any] = {"rollout/episodes": int(state.total_episodes)}
    if not rets:
        out.update({k: None for k in EPISODE_KEYS})
        return out
    out["rollout/ep_rew_mean"] = float(np.mean([round(r, 6) for r in rets]))
    out["rollout/ep_len_mean"] = float(np.mean(lens))
    out["rollout/success_rate"] = float(np.mean(succ))
    return out


def explained_variance(var_y: float, var_diff: float) -> float:
    """stable_baselines3.common.utils.explained_variance from its two variances: nan when var(y_true) is 0"""
    return float("nan") if var_y == 0 else 1.0 - var_diff / var_y


class EpisodeMonitor:
    """The device handle (kp1_monitor): K replicas x N envs.  ``observe`` takes torch tensors [T, K N] (f32 rewards, u8 done bytes) on the
    handle's device and launches on the current stream; nothing comes back to the host before ``read``."""

    def __init__(self, device: Any, n_replicas: int, n_per_replica: int, *, window: int = DEFAULT_WINDOW, max_steps: int) -> None:
        import torch

        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.K, self.N, self.window, self.max_steps = int(n_replicas), int(n_per_replica), int(window), int(max_steps)
        self.L = native.load()
        self._h = C.c_void_p()
        native.check(self.L.kp1_monitor_create(native.device_index(self.device), self.K, self.N, self.window, self.max_steps, C.byref(self._h)))

    def _stream(self) -> C.c_void_p:
        return native.stream_arg(self.device)

    def observe(self, rewards: Any, dones: Any, T: int | None = None) -> None:
        import torch

        if rewards.dtype != torch.float32 or dones.dtype != torch.uint8 or not rewards.is_contiguous() or not dones.is_contiguous():
            raise ValueError("EpisodeMonitor.observe takes contiguous float32 rewards and uint8 done bytes")
        steps = int(rewards.shape[0]) if T is None else int(T)
        if rewards.numel() < steps * self.K * self.N or dones.numel() < steps * self.K * self.N:
            raise ValueError(f"EpisodeMonitor.observe: the buffers hold fewer than {steps} x {self.K * self.N} elements")
        native.check(self.L.kp1_monitor_observe(self._h, native.ptr(rewards), native.ptr(dones), steps, self._stream()))

    def reset_carry(self) -> None:
        native.check(self.L.kp1_monitor_reset_carry(self._h, self._stream()))

    def read(self, replica: int = 0) -> native.MonitorState:
        out = native.MonitorState()
        native.check(self.L.kp1_monitor_read(self._h, int(replica), C.byref(out), self._stream()))
        return out

    def close(self) -> None:
        if self._h:
            self.L.kp1_monitor_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self) -> None:  # pragma: no cover
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


def _cell(value: Any) -> str:
    """a CSV cell as CSVOutputFormat writes it: str(value), empty for a key without a value"""
    if value is None:
        return ""
    if isinstance(value, float):
        return repr(value)
    return str(value)


def _table_value(value: Any) -> str:
    """HumanOutputFormat: floats as %-8.3g, everything else str()"""
    if isinstance(value, float):
        return f"{value:<8.3g}".strip()
    return str(value)


def format_table(row: dict[str, Any]) -> str:
    """SB3's boxed stdout table (HumanOutputFormat.write): keys grouped under their ``tag/`` and indented, keys without a value left out"""
    lines: list[tuple[str, str]] = []
    tag = ""
    for key in sorted(k for k, v in row.items() if v is not None):
        name = key
        if "/" in key:
            head = key[:key.index("/") + 1]
            if head != tag:
                tag = head
                lines.append((tag, ""))
            name = "   " + key[len(tag):]
        lines.append((name[:36], _table_value(row[key])[:36]))
    if not lines:
        return ""
    kw, vw = max(len(k) for k, _ in lines), max(len(v) for _, v in lines)
    dashes = "-" * (kw + vw + 7)
    body = [f"| {k}{' ' * (kw - len(k))} | {v}{' ' * (vw - len(v))} |" for k, v in lines]
    return "\n".join([dashes, *body, dashes])


class TrainLogger:
    """One run's (or one replica's) SB3 record per logged iteration: ``log(stats, iteration=, total_timesteps=)`` completes ``stats`` (the
    rollout/ and train/ keys, e.g. one dict of ``PPO.monitor_rows()``) with the time/ keys, prints the table to ``out`` and appends a row to
    ``csv_path``.  The clock and the step count fps is measured from start at construction or at
    ``restart``."""

    def __init__(self, csv_path: str | Path | None = None, *, out: TextIO | None = None, start_timesteps: int = 0) -> None:
        self.csv_path = Path(csv_path) if csv_path is not None else None
        self.out = out
        self._header_written = False
        self.restart(start_timesteps)

    def restart(self, start_timesteps: int = 0) -> None:
        self._t0 = time.time()
        self._start_steps = int(start_timesteps)

    def row(self, stats: dict[str, Any], *, iteration: int, total_timesteps: int) -> dict[str, Any]:
        elapsed = max(time.time() - self._t0, sys.float_info.epsilon)
        row: dict[str, Any] = {k: None for k in KEYS}
        row.update({k: v for k, v in stats.items() if k in row})
        row.update({"time/fps": int((int(total_timesteps) - self._start_steps) / elapsed), "time/iterations": int(iteration),
                    "time/time_elapsed": int(elapsed), "time/total_timesteps": int(total_timesteps)})
        return row

    def log(self, stats: dict[str, Any], *, iteration: int, total_timesteps: int) -> dict[str, Any]:
        row = self.row(stats, iteration=iteration, total_timesteps=total_timesteps)
        stop = stats.get("kl_stop")
        if stop:      # SB3's PPO.train() (verbose >= 1), for an update that target_kl ended early
            print(f"Early stopping at step {stop['stop_epoch']} due to reaching max kl: {stop['stop_kl']:.2f}", file=self.out or sys.stdout, flush=True)
        print(format_table(row), file=self.out or sys.stdout, flush=True)
        if self.csv_path is not None:
            self.csv_path.parent.mkdir(parents=True, exist_ok=True)
            with self.csv_path.open("a" if self._header_written else "w", encoding="utf-8") as f:
                if not self._header_written:
                    f.write(",".join(KEYS) + "\n")
                    self._header_written = True
                f.write(",".join(_cell(row[k]) for k in KEYS) + "\n")
        return row


def parse_csv_row(header: str, line: str) -> dict[str, Any]:
    """a progress.csv line back into a record: empty cells are None, integer keys ints, the rest floats"""
    ints = {"rollout/episodes", "time/fps", "time/iterations", "time/time_elapsed", "time/total_timesteps", "train/n_updates"}
    out: dict[str, Any] = {}
    for key, cell in zip(header.strip().split(","), line.rstrip("\n").split(",")):
        out[key] = None if cell == "" else (int(cell) if key in ints else float(cell))
    return out


def add_cli_flags(parser: Any) -> None:
    """the trainers' two flags"""
    parser.add_argument("--monitor", action="store_true",
                        help="keep SB3's episode and update statistics on the device (rollout/ep_rew_mean, ep_len_mean, train/explained_variance, "
                             "train/std, ...), print SB3's table at the logging cadence and append to <artifact-root>/progress.csv (one per replica "
                             "with --seeds); single process only")
    parser.add_argument("--stats-window-size", type=int, default=DEFAULT_WINDOW,
                        help=f"with --monitor: episodes the rollout/ means run over (SB3's stats_window_size, default {DEFAULT_WINDOW})")


def cli_monitor(args: Any) -> Any:
    """the ``monitor=`` argument the two flags ask for (False without --monitor); a window out of range is refused here, on the host"""
    if not getattr(args, "monitor", False):
        return False
    return window_of(int(args.stats_window_size))

