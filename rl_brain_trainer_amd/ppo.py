"""PPO rollout-and-update loop on one MI355X (or one rank of a data-parallel job).

Restates stable_baselines3.PPO("MultiInputPolicy") as the reference drives it
(kinematic_phase1/train_workspace_expansion.py:175-232, training/train_dock_policy.py:86-102):

* policy: CombinedExtractor (56 floats, alphabetical key order) -> separate tanh MLPs ``pi`` / ``vf``
  (SB3 default 2x64; BASELINE config 2 asks 2x256) -> ``action_net`` (7) / ``value_net`` (1),
  state-independent ``log_std`` (init 0), orthogonal init (gain sqrt2 / 0.01 / 1);
* rollout: sample a ~ N(mean, exp(log_std)), store the unclipped action, clip to [-1, 1] for the env,
  bootstrap truncated episodes with gamma * V(terminal_observation), GAE(lambda);
* update: n_epochs x shuffled minibatches, per-minibatch advantage normalisation, clipped surrogate +
  0.5 * MSE value loss - ent_coef * entropy, global grad-norm clip 0.5, Adam(eps=1e-5).

SB3 itself is not in the reference tree nor in this image: these semantics are "parity unpinned"
 and are tested against plain-PyTorch references of each op.

Everything stays on the device: the env kernel writes straight into the rollout buffer, the curriculum
tracker is a device kernel, and the only host synchronisation per iteration is the logging read-back.
Under torch.distributed (backend "nccl" = RCCL) env ranges are sharded by rank and gradients are summed
with one flat all-reduce per optimiser step.

``PPO`` is the engine of every trainer: rollout loop, graph capture, rollout tail (``_post_rollout``), minibatch
advantage statistics (``_epoch_adv_stats``) and optimiser step (``_hip_minibatch_step``) stand here once, for one run and for a population.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import time
from dataclasses import dataclass, field
from typing import Any

import numpy as np
import torch

from . import config as kcfg
from . import native
from .curriculum import PointCurriculum
from .vec_env import ArmKinematicVecEnv

OBS_DIM = kcfg.OBS_DIM
ACT_DIM = kcfg.NJ


@dataclass
class PPOConfig:
    """algorithms.ppo block of the YAML (ppo_default.yaml) + SB3 defaults for what the YAML leaves out."""

    learning_rate: float = 3e-4
    n_steps: int = 2048
    batch_size: int = 256
    n_epochs: int = 10
    gamma: float = 0.99
    gae_lambda: float = 0.95
    clip_range: float = 0.2
    ent_coef: float = 0.0
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    adam_eps: float = 1e-5
    seed: int = 0
    hidden: int = 64            # SB3 default net_arch = dict(pi=[64, 64], vf=[64, 64])
    normalize_advantage: bool = True
    total_timesteps: int = 100_000
    # SB3's LinearSchedule for the learning rate / the clip range: {end, end_fraction}, the value running from
    # `learning_rate` / `clip_range` (the start, which --learning-rate, --sweep and "the YAML learning rate wins on resume" keep addressing)
    # to `end` over the first `end_fraction` of the run.  None: a constant, and then nothing differs from a build without them.
    # Keyword-only: in the constructor they stand behind target_kl, so positional use of every other field is unchanged.  Hence
    # dataclasses.fields / astuple list them in front of target_kl, not in the constructor's order; nothing here relies on either order
    learning_rate_schedule: dict | None = field(default=None, kw_only=True)
    clip_range_schedule: dict | None = field(default=None, kw_only=True)
    # SB3's target_kl: train() leaves its epochs once a minibatch's approx_kl exceeds 1.5 * target_kl (None: never).  Decided on the device
    # (DESIGN section 35); last, so positional use of the fields above is unchanged
    target_kl: float | None = None

    @classmethod
    def from_algo_kwargs(cls, kwargs: dict[str, Any], **overrides: Any) -> "PPOConfig":
        known = {f for f in cls.__dataclass_fields__}
        data = {k: v for k, v in kwargs.items() if k in known}
        unknown = set(kwargs) - known
        if unknown:
            raise TypeError(f"PPO.__init__() got unexpected keyword arguments {sorted(unknown)}")
        data.update(overrides)
        return cls(**data)


def param_spec(hidden: int, obs_dim: int = OBS_DIM) -> list[tuple[str, tuple[int, ...]]]:
    """SB3 MultiInputActorCriticPolicy.state_dict() keys/shapes for net_arch pi=vf=[hidden, hidden]; ``obs_dim`` = width of the
    flattened Dict observation (56, or 80 with the route keys of route/route_observation.py:14-61)."""
    H = hidden
    return [
        ("log_std", (ACT_DIM,)),
        ("mlp_extractor.policy_net.0.weight", (H, obs_dim)), ("mlp_extractor.policy_net.0.bias", (H,)),
        ("mlp_extractor.policy_net.2.weight", (H, H)), ("mlp_extractor.policy_net.2.bias", (H,)),
        ("mlp_extractor.value_net.0.weight", (H, obs_dim)), ("mlp_extractor.value_net.0.bias", (H,)),
        ("mlp_extractor.value_net.2.weight", (H, H)), ("mlp_extractor.value_net.2.bias", (H,)),
        ("action_net.weight", (ACT_DIM, H)), ("action_net.bias", (ACT_DIM,)),
        ("value_net.weight", (1, H)), ("value_net.bias", (1,)),
    ]


class ActorCritic:
    """Flat fp32 parameter buffer with SB3-named views."""

    def __init__(self, hidden: int, device: torch.device, seed: int = 0, obs_dim: int = OBS_DIM) -> None:
        self.hidden = hidden
        self.obs_dim = int(obs_dim)
        self.device = device
        self.spec = param_spec(hidden, self.obs_dim)
        self.numel = sum(math.prod(s) for _, s in self.spec)
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=device)
        self.views: dict[str, torch.Tensor] = {}
        off = 0
        for name, shape in self.spec:
            n = math.prod(shape)
            self.views[name] = self.flat[off:off + n].view(shape)
            off += n
        self._init(seed)

    def _init(self, seed: int) -> None:
        g = torch.Generator(device="cpu").manual_seed(int(seed))
        gains = {"mlp_extractor": math.sqrt(2.0), "action_net": 0.01, "value_net": 1.0}
        for name, shape in self.spec:
            if name.endswith("weight"):
                w = torch.empty(shape, dtype=torch.float32)
                torch.nn.init.orthogonal_(w, gain=gains[name.split(".")[0]], generator=g)
                self.views[name].copy_(w)
            else:
                self.views[name].zero_()  # biases and log_std start at 0

    def state_dict(self) -> dict[str, torch.Tensor]:
        return {k: v.detach().clone().cpu() for k, v in self.views.items()}

    def load_state_dict(self, sd: dict[str, torch.Tensor]) -> None:
        for name, shape in self.spec:
            t = sd[name]
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name}: checkpoint shape {tuple(t.shape)} != {tuple(shape)}")
            self.views[name].copy_(t.to(self.device, torch.float32))


def mlp_forward(P: dict[str, torch.Tensor], obs: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """mean[B,7], value[B] of the SB3 MlpExtractor + heads (plain torch; also the reference for the HIP kernels)."""
    hp = torch.tanh(torch.addmm(P["mlp_extractor.policy_net.0.bias"], obs, P["mlp_extractor.policy_net.0.weight"].t()))
    hp = torch.tanh(torch.addmm(P["mlp_extractor.policy_net.2.bias"], hp, P["mlp_extractor.policy_net.2.weight"].t()))
    mean = torch.addmm(P["action_net.bias"], hp, P["action_net.weight"].t())
    hv = torch.tanh(torch.addmm(P["mlp_extractor.value_net.0.bias"], obs, P["mlp_extractor.value_net.0.weight"].t()))
    hv = torch.tanh(torch.addmm(P["mlp_extractor.value_net.2.bias"], hv, P["mlp_extractor.value_net.2.weight"].t()))
    value = torch.addmm(P["value_net.bias"], hv, P["value_net.weight"].t()).squeeze(-1)
    return mean, value


LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def gaussian_log_prob(actions: torch.Tensor, mean: torch.Tensor, log_std: torch.Tensor) -> torch.Tensor:
    z = (actions - mean) * torch.exp(-log_std)
    return (-0.5 * z * z - log_std - LOG_SQRT_2PI).sum(-1)


class GraphSegments:
    """A launch sequence captured as a CHAIN of hipGraphs with eager calls between them (the data-parallel collectives when they are not
    captured themselves).  During capture `cut(fn)` ends the running segment, records `fn` and opens the next one; `replay()` walks the
    chain in capture order on the current stream.  All segments share one memory pool (tensors allocated inside one segment and read by a
    later one, or by a recorded call, keep their addresses; replaying strictly in capture order is what makes sharing the pool safe).
    `on_begin` runs inside every freshly opened capture (the env re-reads the capture stream there)."""

    def __init__(self, device: torch.device, on_begin=None) -> None:
        self.device = device
        self.plan: list[Any] = []
        self.n_graphs = 0
        self._pool = torch.cuda.graph_pool_handle()
        self._on_begin = on_begin
        self._cur = None

    def begin(self) -> None:
        g = torch.cuda.CUDAGraph()
        ctx = torch.cuda.graph(g, pool=self._pool, capture_error_mode="thread_local")
        ctx.__enter__()
        self._cur = (g, ctx)
        if self._on_begin is not None:
            self._on_begin()

    def _end(self) -> None:
        g, ctx = self._cur
        self._cur = None
        ctx.__exit__(None, None, None)
        self.plan.append(g)
        self.n_graphs += 1

    def cut(self, fn) -> None:
        self._end()
        self.plan.append(fn)
        self.begin()

    def finish(self) -> None:
        self._end()

    def abort(self) -> None:
        if self._cur is not None:
            g, ctx = self._cur
            self._cur = None
            try:
                ctx.__exit__(None, None, None)
            except Exception:  # noqa: BLE001 -- already unwinding from the error that made the capture fail
                pass

    def replay(self) -> None:
        for item in self.plan:
            if isinstance(item, torch.cuda.CUDAGraph):
                item.replay()
            else:
                item()


class Dist:
    """torch.distributed glue (backend nccl = RCCL on ROCm, gloo on CPU tests).  world_size 1 = no-ops.

    How the collectives meet the hipGraphs of the rollout and of the update epoch (``graph_mode``):

    * ``"segmented"`` (the default for world_size > 1): the compute between two collectives is captured as one hipGraph segment
      (GraphSegments) and the collectives are launched eagerly between the replays, on the same stream.  Needs nothing from the backend
      (works with gloo), keeps every kernel sequence out of the host's launch path, and costs two graph launches + one collective enqueue
      per optimiser step (~40 us of host time against ~85 us of kernels: the host stays ahead).
    * ``"captured"`` (opt-in, ``KP1_DIST_GRAPHS=1``, nccl only): the RCCL collectives are captured INSIDE the graphs.  No multi-GPU run of
      this path has been recorded yet (the builder has one GPU), so it is not the default; when selected it is probed once per process
      (capture + replay + check of a 4-float all-reduce and a 16-byte all-gather, the verdict all-reduced so every rank takes the same
      path) and a watchdog turns a hang of the probe, of the first real rollout replay or of the first real epoch replay into a process
      exit with a message (never a re-exec); PPO additionally checks after those first replays that all ranks hold identical parameters.
    * single process: plain captured graphs."""

    def __init__(self) -> None:
        import torch.distributed as dist

        self.dist = dist
        # KP1_DIST_FORCE_SINGLE=1 (test hook): a one-rank process group takes the data-parallel code path too, so that the RCCL calls, their
        # stream ordering against the graph segments and the byte all-gather run on a box with one GPU (tests/test_distributed_gpu.py)
        force = os.environ.get("KP1_DIST_FORCE_SINGLE", "0") == "1"
        self.enabled = dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or force)
        self.world_size = dist.get_world_size() if self.enabled else 1
        self.rank = dist.get_rank() if self.enabled else 0
        self.backend = str(dist.get_backend()) if self.enabled else ""
        self._graphs_ok: bool | None = None
        self._segments: GraphSegments | None = None     # set while a segmented capture records: collectives become cut points
        self.rccl = None                                # rccl.RcclComm once use_stream_collectives() has agreed on it
        self.collectives = "torch.distributed" if self.enabled else "none"

    def use_stream_collectives(self, device: torch.device) -> bool:
        """nccl backend: put the training collectives on the LAUNCH stream (rccl.RcclComm: same RCCL, no hop to torch's NCCL stream and back per
        call).  Collective: call on every rank.  Every rank self-tests its communicator and the verdicts are combined through torch.distributed,
        so all ranks take the same path; any failure (library, bootstrap, a wrong sum) leaves the torch.distributed path in place.
        KP1_RCCL_DIRECT=0 switches it off."""
        if not self.enabled or self.backend != "nccl" or self.rccl is not None or os.environ.get("KP1_RCCL_DIRECT", "1") == "0":
            return self.rccl is not None
        import sys
        import threading

        # The bootstrap runs in a helper thread with a deadline: a rank whose ncclCommInitRank does not return (a peer that never arrives) reports
        # "not available" like any other failure and every rank stays on torch.distributed -- a slow path instead of a dead run.
        box: dict[str, Any] = {}

        def boot() -> None:
            try:
                from . import rccl

                torch.cuda.set_device(device)          # the current device is per thread
                box["comm"] = rccl.RcclComm(self.dist, device)
                box["ok"] = box["comm"].self_test()
            except Exception as exc:  # noqa: BLE001 -- whatever goes wrong here, the torch.distributed path is complete by itself
                box["exc"] = exc

        worker = threading.Thread(target=boot, name="kp1-rccl-bootstrap", daemon=True)
        worker.start()
        worker.join(float(os.environ.get("KP1_RCCL_BOOT_SECONDS", "120")))
        comm, ok = box.get("comm"), bool(box.get("ok")) and not worker.is_alive()
        if not ok:
            why = "no answer within the deadline" if worker.is_alive() else (f"{type(box['exc']).__name__}: {box['exc']}" if "exc" in box else "self-test mismatch")
            print(f"[kp1] rank {self.rank}: RCCL on the launch stream not available ({why}); collectives stay on torch.distributed", flush=True, file=sys.stderr)
        verdict = torch.tensor([1.0 if ok else 0.0], device=device)
        self.dist.all_reduce(verdict, op=self.dist.ReduceOp.MIN)
        if verdict.item() > 0.5:
            self.rccl = comm
            self.collectives = "rccl on the launch stream"
        elif comm is not None and not worker.is_alive():
            comm.close()
        return self.rccl is not None

    def close(self) -> None:
        """destroy the launch-stream RCCL communicator (collective in effect: call on every rank, after the last training collective has completed)"""
        if self.rccl is not None:
            self.rccl.close()
            self.rccl = None
            self.collectives = "torch.distributed" if self.enabled else "none"

    def _collective(self, fn) -> None:
        if self._segments is not None:
            self._segments.cut(fn)
        else:
            fn()

    def all_reduce_sum(self, t: torch.Tensor) -> torch.Tensor:
        if self.enabled:
            if self.rccl is not None and t.is_cuda and t.is_contiguous():
                self._collective(lambda: self.rccl.all_reduce_sum(t))
            else:
                self._collective(lambda: self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM))
        return t

    def all_gather_bytes(self, t: torch.Tensor) -> torch.Tensor:
        if not self.enabled:
            return t
        out = torch.empty(self.world_size * t.numel(), dtype=t.dtype, device=t.device)  # rank-major = global env order
        self.dist.all_gather_into_tensor(out, t.contiguous().view(-1))
        return out

    def all_gather_into(self, out: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """out[world, ...] <- every rank's t (rank-major), into a caller-owned buffer (graph replays need a fixed address)."""
        if self.enabled:
            dst, src = out.view(-1), t.contiguous().view(-1)
            if self.rccl is not None and src.is_cuda:
                self._collective(lambda: self.rccl.all_gather(dst, src))
            else:
                self._collective(lambda: self.dist.all_gather_into_tensor(dst, src))
        else:
            out.view(-1).copy_(t.reshape(-1))
        return out

    def broadcast(self, t: torch.Tensor, src: int = 0) -> torch.Tensor:
        if self.enabled:
            self.dist.broadcast(t, src)
        return t

    def graphs_ok(self, device: torch.device) -> bool:
        """True when collectives of this process group can live inside a captured hipGraph (single process: trivially)."""
        if not self.enabled:
            return True
        if self._graphs_ok is None:
            self._graphs_ok = self._probe_graph_collectives(device)
        return self._graphs_ok

    def graph_mode(self, device: torch.device) -> str:
        """"captured" (collectives inside the graphs; always so for a single process) or "segmented" (graph segments, eager collectives)"""
        return "captured" if self.graphs_ok(device) else "segmented"

    def watchdog(self, seconds: float, what: str):
        """arm a timer that ends the process (exit code 3, a message, no re-exec) if `what` has not finished; returns the timer to cancel"""
        import os
        import sys
        import threading

        def _hung() -> None:
            print(f"[kp1] {what} did not complete within {seconds:.0f} s: re-run with KP1_DIST_GRAPHS=0 KP1_RCCL_DIRECT=0 (segmented graphs, torch.distributed collectives)",
                  file=sys.stderr, flush=True)
            os._exit(3)

        dog = threading.Timer(seconds, _hung)
        dog.daemon = True
        dog.start()
        return dog

    def ranks_agree(self, flat: torch.Tensor) -> bool:
        """every rank holds bit-identical `flat` (digest min == max over ranks); a collective itself, call it on all ranks"""
        if not self.enabled:
            return True
        d = flat.double()
        digest = torch.stack([d.sum(), d.abs().sum(), d[::97].sum()])
        lo, hi = digest.clone(), digest.clone()
        self.dist.all_reduce(lo, op=self.dist.ReduceOp.MIN)
        self.dist.all_reduce(hi, op=self.dist.ReduceOp.MAX)
        return bool(torch.equal(lo, hi)) and bool(torch.isfinite(digest).all())

    def _probe_graph_collectives(self, device: torch.device) -> bool:
        import os
        import sys
        import threading

        ok = self.backend == "nccl" and os.environ.get("KP1_DIST_GRAPHS", "0") == "1"   # opt-in: see the class docstring
        verdict = torch.tensor([1.0 if ok else 0.0], device=device)
        if ok:
            buf = torch.full((4,), float(self.rank + 1), device=device)
            expect = float(self.world_size * (self.world_size + 1) // 2)
            # the two collectives the captured graphs contain: the flat gradient all-reduce (update epoch) and the done-byte all-gather (rollout)
            mine = torch.full((16,), self.rank + 1, dtype=torch.uint8, device=device)
            gathered = torch.zeros((self.world_size, 16), dtype=torch.uint8, device=device)
            self.dist.all_reduce(buf.clone())          # communicator fully set up before any capture
            self.dist.all_gather_into_tensor(gathered.clone().view(-1), mine)
            torch.cuda.synchronize(device)

            def _hung() -> None:
                print("[kp1] a captured RCCL all-reduce did not complete within 120 s: re-run with KP1_DIST_GRAPHS=0", file=sys.stderr, flush=True)
                os._exit(3)

            dog = threading.Timer(120.0, _hung)
            dog.daemon = True
            dog.start()
            g, good = None, True
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self.dist.all_reduce(buf)
                    self.dist.all_gather_into_tensor(gathered.view(-1), mine)
            except Exception as exc:  # noqa: BLE001 -- capture of a collective is refused in many ways depending on the build
                print(f"[kp1] rank {self.rank}: RCCL inside hipGraph capture not available ({type(exc).__name__}: {exc}); eager collectives", file=sys.stderr)
                good = False
            # a rank whose capture failed never replays: agree (eagerly) that EVERY rank captured before any rank replays
            captured = torch.tensor([1.0 if good else 0.0], device=device)
            self.dist.all_reduce(captured, op=self.dist.ReduceOp.MIN)
            good = bool(captured.item() > 0.5)
            if good:
                buf.fill_(float(self.rank + 1))
                gathered.zero_()
                g.replay()
                torch.cuda.synchronize(device)
                want = torch.arange(1, self.world_size + 1, dtype=torch.uint8, device=device)[:, None].expand(-1, 16)
                good = bool(torch.all(buf == expect).item()) and bool(torch.equal(gathered, want))
            dog.cancel()
            verdict.fill_(1.0 if good else 0.0)
        self.dist.all_reduce(verdict, op=self.dist.ReduceOp.MIN)   # every rank takes the same path
        return bool(verdict.item() > 0.5)


def _bind_policy(policy: ActorCritic, flat: torch.Tensor) -> None:
    """make `policy` a view on row `flat` of a population's [K, P] parameter buffer (values copied in first)"""
    flat.copy_(policy.flat)
    policy.flat = flat
    off = 0
    for name, shape in policy.spec:
        n = math.prod(shape)
        policy.views[name] = flat[off:off + n].view(shape)
        off += n


def load_adam_state(opt: dict[str, Any], spec, adam_m: torch.Tensor, adam_v: torch.Tensor) -> tuple[int, int]:
    """``policy.optimizer.pth`` state into the flat first / second moments; returns (common step count, extra steps of the actor tensors)"""
    steps, off = [], 0
    for i, (name, shape) in enumerate(spec):
        n = math.prod(shape)
        st = opt["state"].get(i)
        if st is None or tuple(st["exp_avg"].shape) != tuple(shape):
            raise ValueError(f"optimizer state of parameter {i} ({name}) does not match the policy")
        adam_m[off:off + n].copy_(st["exp_avg"].to(adam_m.device, torch.float32).reshape(-1))
        adam_v[off:off + n].copy_(st["exp_avg_sq"].to(adam_v.device, torch.float32).reshape(-1))
        steps.append((name, int(float(st["step"]))))
        off += n
    actor = [s_ for n_, s_ in steps if n_.startswith(("mlp_extractor.policy_net", "action_net"))]
    rest = [s_ for n_, s_ in steps if not n_.startswith(("mlp_extractor.policy_net", "action_net"))]
    if len(set(actor)) != 1 or len(set(rest)) != 1 or actor[0] < rest[0]:
        raise ValueError(f"unsupported per-tensor Adam step pattern {steps}")
    return rest[0], actor[0] - rest[0]


def restore_saved_hyperparameters(cfg: "PPOConfig", data: dict[str, Any]) -> dict[str, Any]:
    """the algorithm constants a loaded SB3 model keeps (see PPO.load_checkpoint) into cfg; returns what was taken"""
    taken = {}
    for key, cast in (("gamma", float), ("gae_lambda", float), ("ent_coef", float), ("vf_coef", float), ("max_grad_norm", float),
                      ("n_epochs", int), ("normalize_advantage", bool)):
        v = data.get(key)
        if isinstance(v, (int, float, bool)) and not (isinstance(v, bool) and cast is not bool):
            setattr(cfg, key, cast(v))
            taken[key] = cast(v)
    clip = data.get("clip_range")
    if isinstance(clip, dict) and isinstance(clip.get("value"), (int, float)):   # this engine's writer; SB3 pickles the schedule
        cfg.clip_range = float(clip["value"])
        taken["clip_range"] = cfg.clip_range
    return taken


# The widths kp1_mlp_forward_env_step covers: 256 (the tile kernels' rollout form), 64 / 128 (rollout_step_kernel)
FUSED_ROLLOUT_WIDTHS = (64, 128, 256)


def check_target_kl(targets: list[float | None], dist: Any, teacher_anchor: Any = None) -> list[float | None]:
    """The refusals of ``target_kl`` (one entry per replica) before any device work.  Returns the targets with "no target" as None: None,
    NaN and values <= 0 (what the handle takes as none).  A KL stop is a per-process decision -- under data parallel the ranks would leave
    an update at different minibatches and diverge, and SB3 has no counterpart -- and the teacher-anchor step reads the one shared Adam
    count that a gated handle no longer keeps."""
    out = [None if t is None or not float(t) > 0.0 else float(t) for t in targets]
    if any(t is not None for t in out):
        if dist is not None and getattr(dist, "enabled", False):
            raise ValueError("target_kl is not supported under data parallel: each rank would stop on its own shard's KL and the ranks would diverge")
        if teacher_anchor is not None:
            raise ValueError("target_kl is not supported together with a teacher anchor: the anchor step reads the shared Adam step count")
    return out


SCHEDULE_KEYS = ("end", "end_fraction")


def linear_schedule(start: float, end: float, end_fraction: float, progress_remaining: float) -> float:
    """stable_baselines3.common.utils.LinearSchedule(start, end, end_fraction)(progress_remaining), in Python floats (restated from SB3 2.8;
    parity unpinned)"""
    if (1 - progress_remaining) > end_fraction:
        return end
    return start + (1 - progress_remaining) * (end - start) / end_fraction


def check_schedule(name: str, sched: Any, *, end_may_be_zero: bool) -> dict[str, float] | None:
    """one ``PPOConfig.*_schedule`` mapping as {end, end_fraction} floats, or None (unset).  ValueError: not a mapping, unknown or missing
    keys, non-finite values, end_fraction outside (0, 1], a negative end (``end_may_be_zero``: the learning rate may reach 0, the clip
    range must stay positive)."""
    if sched is None:
        return None
    if not isinstance(sched, dict):
        raise ValueError(f"{name} must be a mapping {{end, end_fraction}} (got {type(sched).__name__})")
    unknown, missing = sorted(set(sched) - set(SCHEDULE_KEYS)), [k for k in SCHEDULE_KEYS if k not in sched]
    if unknown:
        raise ValueError(f"{name} has unknown keys {unknown}: a schedule is {{end, end_fraction}}, its start is the field it anneals")
    if missing:
        raise ValueError(f"{name} needs the keys {list(SCHEDULE_KEYS)} (missing {missing})")
    try:
        end, frac = float(sched["end"]), float(sched["end_fraction"])
    except (TypeError, ValueError):
        raise ValueError(f"{name} needs numbers for end and end_fraction (got {sched!r})") from None
    if not (math.isfinite(end) and math.isfinite(frac)):
        raise ValueError(f"{name} must be finite (got {sched!r})")
    if not 0.0 < frac <= 1.0:
        raise ValueError(f"{name}: end_fraction must lie in (0, 1] (got {frac!r})")
    if end < 0.0 or (end == 0.0 and not end_may_be_zero):
        raise ValueError(f"{name}: end must be {'>= 0' if end_may_be_zero else '> 0'} (got {end!r})")
    return {"end": end, "end_fraction": frac}


def check_schedules(cfg: "PPOConfig", teacher_anchor: Any = None) -> dict[str, dict[str, float]] | None:
    """The refusals of ``learning_rate_schedule`` / ``clip_range_schedule`` before any device work.  Returns {field: {end, end_fraction}} of
    the schedules set, or None when both are unset.  The reference's teacher-anchor callback steps with whatever learning rate the
    optimiser last held; that is not restated, so an anchor together with a schedule is refused."""
    out = {}
    for fld, zero_ok in (("learning_rate", True), ("clip_range", False)):
        s = check_schedule(f"{fld}_schedule", getattr(cfg, f"{fld}_schedule", None), end_may_be_zero=zero_ok)
        if s is not None:
            out[fld] = s
    if out and teacher_anchor is not None:
        raise ValueError("a learning-rate / clip-range schedule is not supported together with a teacher anchor: the anchor step's learning "
                         "rate under a schedule is not restated")
    return out or None


def fused_rollout_covered(env_type_ok: bool, dtype: Any, hidden: int, obs_dim: int, components_on: bool, env_var: str | None, *,
                          default_on: bool = True) -> bool:
    """Whether a rollout step runs as ONE launch (policy forward + sampling + env step with auto-reset) instead of forward + step_into.
    ``env_type_ok``: the env is one the entry point steps (the plain fp32 vectorised env, or an Approach / dock population env on one
    handle); ``dtype``: the env's real type; ``obs_dim``: 56 is covered, the 80-float route observation is not; ``components_on``: recorded
    reward components need the env's own step kernel; ``env_var``: KP1_FUSED_ROLLOUT ("0": the launch sequence, kept as the A/B and test
    reference; any other value: the one-launch form wherever it exists; None = unset: ``default_on``, the calling trainer's measured
    default -- on only where its rollout beat the launch sequence by more than the run-to-run spread)."""
    if not env_type_ok or dtype != torch.float32 or hidden not in FUSED_ROLLOUT_WIDTHS or obs_dim > 64 or components_on:
        return False
    return bool(default_on) if env_var is None else env_var != "0"


# kp1_rollout_run: all env steps of a rollout in one launch per span
ROLLOUT_RUN_ENV = "KP1_ROLLOUT_RUN"
ROLLOUT_RUN_WIDTHS = (64, 128)
ROLLOUT_RUN_TRACKED_MAX_ENVS = 32      # a tracked replica must be one 32-row tile


def rollout_run_covered(step_covered: bool, hidden: int, mode_name: str, dist_enabled: bool, has_step_callback: bool, tracker_attached: bool,
                        envs_per_replica: int, env_var: str | None, *, tracker_ok: bool = True, default_on: bool = False) -> bool:
    """Whether a rollout runs as ONE launch per span of env steps (``MlpKernels.rollout_run``, plus one launch for the critic) instead of
    the per-step loop.  ``step_covered``: the configuration is one the one-launch step covers (fused_rollout_covered: env type, fp32, the
    56-float observation, reward components off); ``hidden``: 64 / 128 (hidden 256, the tile path, keeps its step); ``mode_name``: approach
    only; ``dist_enabled``: a data-parallel run exchanges done bytes per chunk and keeps the loop; ``has_step_callback``: a host hook after
    every step keeps the loop; ``tracker_attached`` / ``envs_per_replica``: the launch runs the tracker itself only when a replica is one tile
    (at most ROLLOUT_RUN_TRACKED_MAX_ENVS envs); ``tracker_ok``: the attached tracker's ``runs_in_rollout_launch`` (the point trackers');
    ``env_var``: KP1_ROLLOUT_RUN ("0": the per-step loop; any other value: the whole-rollout form wherever it is covered; None = unset:
    ``default_on``, the calling trainer's default -- off everywhere until a measurement by DESIGN section 27's rule turns it on)."""
    if not step_covered or hidden not in ROLLOUT_RUN_WIDTHS or mode_name != "approach" or dist_enabled or has_step_callback:
        return False
    if tracker_attached and (not tracker_ok or envs_per_replica > ROLLOUT_RUN_TRACKED_MAX_ENVS):
        return False
    return bool(default_on) if env_var is None else env_var != "0"


# KP1_MLP_OPT_TRAIN_TILE: the optimiser step's forward, loss and backward as one tile launch at the layer-wise widths
TRAIN_TILE_WIDTHS = (64, 128)
TRAIN_TILE_ENV = "KP1_TRAIN_TILE"
TRAIN_TILE_MAX_ROWS = 2048             # csrc/kp1_train_tile.inc TT_MAX_ROWS: 64 chunks of one 32-row tile


def train_tile_covered(hidden: int, env_var: str | None, *, default_on: bool = False) -> bool:
    """Whether a trainer switches ``MlpKernels.set_train_tile`` on.  ``hidden``: 64 / 128 (hidden 256 has its own tile path); ``env_var``:
    KP1_TRAIN_TILE, "1" is on and any other value off; None = unset: ``default_on``, the trainer's default (off until a measurement by
    DESIGN section 20's rule turns it on)."""
    if hidden not in TRAIN_TILE_WIDTHS:
        return False
    return bool(default_on) if env_var is None else env_var == "1"


def train_tile_chunks(n: int) -> int:
    """Chunks (= 32-row tiles) of an n-row minibatch under KP1_MLP_OPT_TRAIN_TILE, or 0: the layer-wise launches take it
    (csrc/kp1_train_tile.inc train_tile_chunks).  A function of n alone."""
    return (n + 31) // 32 if 1 <= n <= TRAIN_TILE_MAX_ROWS else 0


# kp1_mlp_forward_route_step: the widths, the observation widths and the route length it covers
FUSED_ROUTE_ROLLOUT_WIDTHS = (64, 128)
FUSED_ROUTE_ROLLOUT_OBS_DIMS = (56, 80)
ROUTE_FUSED_MAX_WAYPOINTS = native.header_int("KP1_ROUTE_FUSED_MAX_WAYPOINTS")
FUSED_ROUTE_ROLLOUT_ENV = "KP1_FUSED_ROUTE_ROLLOUT"


def fused_route_rollout_covered(env_type_ok: bool, dtype: Any, hidden: int, obs_dim: int, components_on: bool, n_waypoints: int,
                                dist_enabled: bool, env_var: str | None) -> bool:
    """Whether a rollout step on a ROUTE env runs as ONE launch (``MlpKernels.forward_route_step``) instead of forward + step_into.  Opt-in:
    ``env_var`` is KP1_FUSED_ROUTE_ROLLOUT, and unset or "0" is the launch sequence (KP1_FUSED_ROLLOUT, the arm envs' switch, is never
    consulted here).  Covered: a RouteVecEnv / RoutePopulationVecEnv (``env_type_ok``) at fp32, hidden 64 / 128, the 56- or 80-float
    observation, reward components off, a route of at most ROUTE_FUSED_MAX_WAYPOINTS waypoints, and a run that is not data parallel."""
    if env_var is None or env_var == "0":
        return False
    if not env_type_ok or dtype != torch.float32 or hidden not in FUSED_ROUTE_ROLLOUT_WIDTHS or obs_dim not in FUSED_ROUTE_ROLLOUT_OBS_DIMS:
        return False
    if components_on or dist_enabled or n_waypoints > ROUTE_FUSED_MAX_WAYPOINTS:
        return False
    return True


def truncation_cap(n_steps: int, n_envs: int, env: Any) -> int:
    """Rows per replica of the time-limit bootstrap's index list.  Only truncated steps need the critic, and an env truncates at most
    n_steps // max_episode_steps + 1 times per rollout, so a replica's truncated positions fit a list of this fixed size
    (torch.nonzero_static: no device->host size query)."""
    return min(n_envs * (n_steps // max(int(env.config.c.termination.max_episode_steps), 1) + 1), n_steps * n_envs)


class PPO:
    """One PPO run.  PopulationPPO (population.py) is the same engine with K replicas: everything per replica below is a list (``envs``,
    ``curricula``, ``policies``, ``gens``) or a replica axis (rollout columns [k N, (k + 1) N), ``perm[k]``, ``stats_dev[k]``); here K = 1.
    A trainer class overrides ``_rollout_env``, ``_rollout_tracker``, the type predicates and, if it must, ``_gae_scan``,
    ``_bootstrap_truncated``, ``_draw_noise`` and ``_epoch_body``'s index preparation; never the rollout tail or the optimiser step."""

    # the training monitor (monitor.py): None = off, the default, and then no launch, graph or printed line differs from a build without it
    monitor = None
    _monitor_live = True

    def __init__(self, env: ArmKinematicVecEnv, cfg: PPOConfig, *, curriculum: PointCurriculum | None = None,
                 dist: Dist | None = None, backend: str = "hip", use_graphs: bool = True, monitor: bool | int = False) -> None:
        """``monitor``: False (off), True (SB3's episode and update statistics on the device, over the newest 100 episodes) or that
        window; fixed at construction, read with ``monitor_rows()``"""
        if backend != "hip":
            raise ValueError("backend must be 'hip': the HIP kernels are the only training path")
        if getattr(env, "is_population", False):
            raise TypeError("PPO trains one seed; a population env (K replicas in one handle) is trained by population.ApproachPopulationPPO")
        if env.dtype != torch.float32:
            raise ValueError("PPO drives the production f32 env")
        dist = dist or Dist()
        from . import monitor as _monitor

        _monitor.check_monitor(monitor, dist)     # a data-parallel run is refused before any device work
        targets = check_target_kl([cfg.target_kl], dist)
        schedules = check_schedules(cfg)
        self.env = env
        self.curriculum = curriculum
        self._setup(cfg, [cfg.seed], [env], [curriculum], dist, use_graphs, min_batch=8192, stacked=False, monitor=monitor)
        self.policy = self.policies[0]
        self._trunc_cap = truncation_cap(cfg.n_steps, self.n_envs, env)
        self._setup_kl_gate(targets)
        self._setup_schedules(schedules)
        T, N, dev = cfg.n_steps, self.n_envs, self.device
        # data parallel: done bytes are exchanged once per `done_chunk` env steps (one all-gather of chunk x N bytes instead of one
        # latency-bound collective per 45 us env step); the device tracker replays the chunk in the reference's order
        self.done_chunk = 1
        if self.dist.enabled:
            self.done_chunk = math.gcd(T, max(int(os.environ.get("KP1_DONE_EXCHANGE_STEPS", "16")), 1))
            self._done_gather = torch.zeros((self.dist.world_size, self.done_chunk, N), dtype=torch.uint8, device=dev)
            # a route tracker also reads per-env flags that every step overwrites: each step's episode records are staged in slot t % chunk
            # and the staging buffer is exchanged instead of the done bytes
            self._record_stage = None
            if curriculum is not None and curriculum.needs_episode_records:
                self._record_stage = torch.zeros((self.done_chunk, N), dtype=torch.uint8, device=dev)

    @property
    def _fused_env_step(self) -> bool:
        """whether the next rollout step is the one-launch form (fused_rollout_covered on the env's current state: the reward-component
        switch may be thrown after construction, which bumps ``launch_args_version`` and re-captures the rollout)"""
        return fused_rollout_covered(*self._step_coverage(), os.environ.get("KP1_FUSED_ROLLOUT"), default_on=self._fused_rollout_default())

    def _step_coverage(self) -> tuple[bool, Any, int, int, bool]:
        """what fused_rollout_covered asks about the run's current state: the env handle's type and real type, the two widths, whether
        reward components are recorded"""
        env = self._rollout_env()
        return self._rollout_env_type_ok(), env.dtype, self.cfg.hidden, self.obs_dim, getattr(env, "_reward_components_on", False)

    def _fused_rollout_default(self) -> bool:
        """the one-launch step while KP1_FUSED_ROLLOUT is unset: hidden 256 (measured); the single-seed PPO at hidden
        64 / 128 was not measured and opts in with KP1_FUSED_ROLLOUT=1"""
        return self.cfg.hidden == 256

    # the trainer's default for the one-launch training tile while KP1_TRAIN_TILE is unset: off until a measurement by DESIGN section 20's
    # rule turns it on
    train_tile_default = False

    @property
    def update_form(self) -> str:
        """which kernels the optimiser step's forward / loss / backward runs: recorded in training_summary.json"""
        if self.cfg.hidden == 256:
            return "tile 2x256 (mlp_tile_kernel)" if self._mlp.fused else "layer-wise"
        return "train tile (train_tile128_kernel)" if self._mlp.train_tile else "layer-wise"

    # the trainer's default for the whole-rollout form while KP1_ROLLOUT_RUN is unset: off until a measurement by DESIGN section 27's rule
    # turns it on
    whole_rollout_default = False

    @property
    def _whole_rollout(self) -> bool:
        """whether the next rollout is ONE launch per span of env steps (rollout_run_covered on the run's current state).  KP1_ROLLOUT_RUN is
        read first: unset (and off by default) or "0", nothing else is looked at."""
        var = os.environ.get(ROLLOUT_RUN_ENV)
        if var == "0" or (var is None and not self.whole_rollout_default):
            return False
        env, cur = self._rollout_env(), self._rollout_tracker()
        step_covered = fused_rollout_covered(*self._step_coverage(), None, default_on=True)
        return rollout_run_covered(step_covered, self.cfg.hidden, getattr(env, "_mode_name", ""), self.dist.enabled, self.step_callback is not None,
                                   cur is not None, self.n_envs, var, tracker_ok=cur is not None and cur.runs_in_rollout_launch,
                                   default_on=self.whole_rollout_default)

    # The env handle and the tracker of a rollout step, and which one-launch forms that handle's type admits: all that differs between
    # this class and a one-handle population (population.OneHandlePopulationPPO) in the rollout step below.
    def _rollout_env(self) -> Any:
        """the env handle a rollout step steps"""
        return self.env

    def _rollout_tracker(self) -> Any:
        """the tracker that follows every env step (None: no tracker attached)"""
        return self.curriculum

    def _rollout_env_type_ok(self) -> bool:
        """an env kp1_mlp_forward_env_step / kp1_rollout_run step: the plain arm env, no subclass"""
        return type(self.env) is ArmKinematicVecEnv

    def _route_env_type_ok(self) -> bool:
        """an env kp1_mlp_forward_route_step steps: a single-seed route env"""
        from .route_env import RoutePopulationVecEnv, RouteVecEnv

        return isinstance(self.env, RouteVecEnv) and not isinstance(self.env, RoutePopulationVecEnv)

    def _rollout_whole(self, n_steps: int | None = None, *, tracked: bool = True) -> None:
        """env steps 0 .. n_steps - 1 (default: the whole rollout) as one launch per span, the attached tracker included"""
        self._mlp.rollout_run(self._rollout_env(), self.obs_buf, noise=self.noise_all, value=self.val_buf, action=self.act_buf,
                              log_prob=self.logp_buf, reward=self.rew_buf, done=self.done_buf, terminal_obs=self.term_obs_buf, first_step=0,
                              n_steps=self.cfg.n_steps if n_steps is None else n_steps, trackers=self._rollout_tracker() if tracked else None,
                              steps_per_call=self.n_envs)

    @property
    def _fused_route_step(self) -> bool:
        """whether the next rollout step is the one-launch ROUTE form (fused_route_rollout_covered; opt-in with KP1_FUSED_ROUTE_ROLLOUT).  The
        variable is read first: without it no attribute of the env is touched."""
        var = os.environ.get(FUSED_ROUTE_ROLLOUT_ENV)
        if var is None or var == "0" or not self._route_env_type_ok():
            return False
        env = self._rollout_env()
        return fused_route_rollout_covered(True, env.dtype, self.cfg.hidden, self.obs_dim, bool(getattr(env, "_reward_components_on", False)),
                                           int(getattr(env, "n_waypoints", 0)), self.dist.enabled, var)

    def _setup(self, cfg: PPOConfig, seeds: list[int], envs: list[Any], curricula: list[Any], dist: Dist, use_graphs: bool, *,
               min_batch: int, stacked: bool, monitor: bool | int = False) -> None:
        """What a run of K = len(seeds) replicas holds.  Replica k owns what PPO(seed=s_k) owns: the env handle envs[k] and its tracker
        curricula[k], the parameter init and the generators of rollout noise and shuffles.  Rollout buffers are [T(+1), K N, ...] with replica
        k's envs in columns [k N, (k + 1) N); one MLP handle with K replicas trains all of them.  ``min_batch``: lower bound of that handle's
        max_batch.  ``stacked``: parameters, Adam moments and gradient are [K, P] (a population, any K) instead of one run's [P]."""
        self.cfg = cfg
        self.dist = dist
        self.backend = "hip"
        self.L = native.load()
        self.K = K = len(seeds)
        self.envs, self.curricula = envs, curricula
        self.device = dev = envs[0].device
        self.n_envs = N = envs[0].n_envs                        # per replica
        self.obs_dim = int(getattr(envs[0], "obs_dim", OBS_DIM))   # 80 for the route envs with include_route_keys
        # observation rows are written with pitch 64 / 128 (zero padded) so the MFMA GEMMs read them directly
        self.obs_w = 64 if self.obs_dim <= 64 else 128
        for env, cur in zip(envs, curricula):
            if cur is not None:
                cur.attach(env)
            env.set_obs_stride(self.obs_w)
        # row k of the [K, P] buffers = what PPO(seed=s_k) holds
        self.policies = [ActorCritic(cfg.hidden, dev, seed=s, obs_dim=self.obs_dim) for s in seeds]
        self.flat = self.policies[0].flat
        if stacked:
            self.flat = torch.zeros((K, self.policies[0].numel), dtype=torch.float32, device=dev)
            for k, pol in enumerate(self.policies):
                _bind_policy(pol, self.flat[k])
        self.dist.broadcast(self.flat)
        self.adam_m = torch.zeros_like(self.flat)
        self.adam_v = torch.zeros_like(self.flat)
        self.grad = torch.zeros_like(self.flat)
        self.stats_dev = torch.zeros((K, 4), dtype=torch.float32, device=dev)
        self.adam_t = 0                # one Adam step count for all replicas
        self.n_train_calls = 0         # train() calls so far: SB3's _n_updates = n_train_calls * n_epochs
        self.actor_extra_steps = 0    # optimiser steps only the actor tensors took (teacher-anchor side updates)
        self.num_timesteps = 0         # per replica
        T, KN = cfg.n_steps, K * N
        self.obs_buf = torch.zeros((T + 1, KN, self.obs_w), dtype=torch.float32, device=dev)
        self.term_obs_buf = torch.zeros((T, KN, self.obs_w), dtype=torch.float32, device=dev)
        self.act_buf = torch.zeros((T, KN, ACT_DIM), dtype=torch.float32, device=dev)
        self.clip_act = torch.zeros((KN, ACT_DIM), dtype=torch.float32, device=dev)
        self.logp_buf = torch.zeros((T, KN), dtype=torch.float32, device=dev)
        self.val_buf = torch.zeros((T, KN), dtype=torch.float32, device=dev)
        self.rew_buf = torch.zeros((T, KN), dtype=torch.float32, device=dev)
        self.done_buf = torch.zeros((T, KN), dtype=torch.uint8, device=dev)
        self.adv_buf = torch.zeros((T, KN), dtype=torch.float32, device=dev)
        self.ret_buf = torch.zeros((T, KN), dtype=torch.float32, device=dev)
        # exploration noise of a whole rollout is drawn in ONE call, graphs or not: the eager and the replayed rollout then consume the
        # generator identically and stay bit-identical (tests/test_distributed_gpu.py compares them)
        self.noise_all = torch.zeros((T, KN, ACT_DIM), dtype=torch.float32, device=dev)
        self.perm = torch.zeros((K, T * N), dtype=torch.int64, device=dev)     # replica k's shuffle of the epoch (the epoch graph reads it)
        self.gens = [torch.Generator(device=dev).manual_seed(int(s) + 7919 * self.dist.rank) for s in seeds]
        self._perm_rngs = [np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(s), self.dist.rank, 0x6B7031]))) for s in seeds]   # shuffle keys
        self._needs_reset = True
        self._last_stats_dev: tuple[torch.Tensor, int] | None = None    # (loss sums of the last train() on the device, number of updates)
        self._last_stats_host: list[dict[str, float]] = [{} for _ in range(K)]
        from . import mlp as _mlp

        local_bs = max(cfg.batch_size // self.dist.world_size, 1)
        self._mlp = _mlp.MlpKernels(cfg.hidden, dev, max_batch=max(N, local_bs, min_batch), obs_dim=self.obs_dim, replicas=K)
        self._mlp.pack(self.flat)
        if os.environ.get("KP1_BF16X3_WGRAD", "0") == "1" and cfg.hidden == 256:
            # round-3 EXPERIMENT (off by default, never used by bench.py's value): weight-gradient GEMMs on bf16 x 3 operands
            self._mlp.set_bf16x3_wgrad(True)
        if train_tile_covered(cfg.hidden, os.environ.get(TRAIN_TILE_ENV), default_on=self.train_tile_default):
            self._mlp.set_train_tile(True)
        # hipGraph replay of the rollout (T x 3 launches) and of one update epoch.  Data parallel: graph segments with eager collectives
        # between them, or (opt-in) the RCCL collectives captured inside the graphs: Dist.graph_mode.
        self.use_graphs = bool(use_graphs)
        self.dist.use_stream_collectives(dev)     # nccl: the training collectives go on the launch stream (rccl.py); else a no-op
        self.graph_mode = self.dist.graph_mode(dev) if self.use_graphs else "none"
        self._first_replay_checked = {"rollout": not (self.dist.enabled and self.graph_mode == "captured"),
                                      "epoch": not (self.dist.enabled and self.graph_mode == "captured")}
        self._rollout_graph = None
        self._epoch_graph = None
        self._epoch_policy = os.environ.get("KP1_DP_EPOCH", "auto")     # segmented mode only: "auto" (measured), "graph", "eager"
        self._epoch_auto = None
        self.epoch_form = "one graph" if self.graph_mode == "captured" else ("eager launches" if self.graph_mode == "none" or self._epoch_policy == "eager" else "graph segments")
        self._rollout_graph_key = None     # (launch_args_version of every env, which trackers are attached, gamma, lambda) the rollout graph froze
        self._epoch_graph_key = None       # hyper-parameters baked into the epoch graph's kernel arguments
        self._epoch_warm = False           # one eager epoch has run (kernel attributes set, code objects loaded) before the epoch graph is captured
        self._kernels_warm = False         # the rollout kernels have run once (code objects loaded, attributes set)
        # optional host hook after every env step (done bits of that step, device tensor): what SB3 callbacks' _on_step sees.
        # Setting it makes the rollout eager (a host hook cannot live inside a hipGraph replay).
        self.step_callback = None
        self._setup_monitor(monitor)

    # ------------------------------------------------------------------ KL early stop (target_kl)
    # None = off, the default, and then no launch, graph or printed line differs from a build without it
    kl_targets: list[float | None] | None = None

    def _setup_kl_gate(self, targets: list[float | None]) -> None:
        """``target_kl`` of every replica (None: that replica never stops).  With any target set the MLP handle gets its gate here, for the
        trainer's life: the update's finalize and Adam launches are then the gated instantiations, the Adam step count lives on the device
        per replica, and what the host needs of a train() call -- the steps taken, the epochs begun, the minibatches that entered the
        statistics -- is read back lazily from the replicas' records (``_resolve_kl``)."""
        if not any(t is not None for t in targets):
            return
        self.kl_targets = list(targets)
        self._mlp.set_kl_gate(self.kl_targets)
        self.adam_steps = [int(self.adam_t)] * self.K            # resolved per-replica Adam step counts
        self.kl_n_updates = [self.n_train_calls * self.cfg.n_epochs] * self.K     # SB3's _n_updates per replica: epochs begun
        self._kl_records: list[dict[str, Any]] = [{} for _ in range(self.K)]     # kl_stops() of the last resolved train() call
        self._kl_pending: Any = None      # the event behind the last train() call while its records are unread
        self._kl_fresh = [False] * self.K     # replicas whose stop the monitor has not reported yet
        self._kl_stream = torch.cuda.Stream(self.device)

    def _resolve_kl(self) -> None:
        """bring the host up to the last train() call: per replica the Adam step count, the epochs begun and the stop record.  Waits for that
        update only (a side stream behind its event), not for launches queued since."""
        if self.kl_targets is None or self._kl_pending is None:
            return
        self._kl_stream.wait_event(self._kl_pending)
        records, steps = self._mlp.kl_gate_read(self._kl_stream)
        self._kl_pending = None
        n_mb = self._n_minibatches()
        for k, (r, st) in enumerate(zip(records, steps)):
            stopped = bool(r["stopped"])
            self._kl_records[k] = {"early_stop": stopped, "stop_epoch": r["stop_index"] // n_mb if stopped else None,
                                   "stop_minibatch": r["stop_index"] % n_mb if stopped else None, "stop_kl": float(r["stop_kl"]) if stopped else None,
                                   "n_counted": int(r["n_counted"])}
            self.kl_n_updates[k] += r["stop_index"] // n_mb + 1 if stopped else self.cfg.n_epochs
            self.adam_steps[k] = st
            self._kl_fresh[k] = stopped
        self.adam_t = self.adam_steps[0]

    def _n_minibatches(self) -> int:
        """optimiser steps per epoch"""
        total = self.cfg.n_steps * self.n_envs
        local_bs = max(self.cfg.batch_size // self.dist.world_size, 1)
        return (total + local_bs - 1) // local_bs

    def kl_stops(self) -> list[dict[str, Any]]:
        """per replica, how the last train() call ended under ``target_kl``: ``early_stop``, and where it stopped (``stop_epoch``,
        ``stop_minibatch``, the minibatch's ``stop_kl``; None without a stop).  Reading it synchronises with that update."""
        if self.kl_targets is None:
            raise RuntimeError("kl_stops needs a trainer whose config sets target_kl")
        self._resolve_kl()
        return [{k: v for k, v in r.items() if k != "n_counted"} for r in self._kl_records]

    def n_updates(self, k: int = 0) -> int:
        """SB3's ``_n_updates`` of replica k: n_epochs per train() call, or the epochs begun where ``target_kl`` ended a call early"""
        if self.kl_targets is None:
            return self.n_train_calls * self.cfg.n_epochs
        self._resolve_kl()
        return self.kl_n_updates[k]

    def adam_step_count(self, k: int = 0) -> int:
        """optimiser steps replica k has taken (torch.optim.Adam's ``step``)"""
        if self.kl_targets is None:
            return int(self.adam_t)
        self._resolve_kl()
        return self.adam_steps[k]

    def _kl_after_load(self) -> None:
        """a restored optimiser state and step clock: every replica continues from them"""
        if self.kl_targets is None:
            return
        self._resolve_kl()
        self.adam_steps = [int(self.adam_t)] * self.K
        self.kl_n_updates = [self.n_train_calls * self.cfg.n_epochs] * self.K

    # ------------------------------------------------------------------ learning-rate / clip-range schedules
    # None = no schedule, the default, and then no launch, graph or archive byte differs from a build without them
    hparam_schedules: dict[str, dict[str, float]] | None = None
    # SB3's _current_progress_remaining: run_training sets it after every rollout; a caller driving collect_rollouts() / train() sets it itself
    progress_remaining: float = 1.0

    def _setup_schedules(self, schedules: dict[str, dict[str, float]] | None) -> None:
        """With a schedule set, every train() call writes the replicas' hyper-parameters of that call into the MLP handle's table with one
        small launch (``_store_scheduled_hparams``) and the update's kernels read them there: the captured epoch graph holds the table's
        address, so a value that changes from iteration to iteration costs neither a synchronisation nor a re-capture."""
        if not schedules:
            return
        self.hparam_schedules = dict(schedules)
        self.scheduled_values: list[dict[str, float]] | None = None     # per replica, what the last train() call used (Python floats)

    def scheduled_hparams(self, k: int = 0) -> dict[str, float]:
        """replica k's learning rate and clip range at ``progress_remaining``: SB3's ``lr_schedule(p)`` / ``clip_range(p)``, in Python floats"""
        c = (getattr(self, "cfgs", None) or [self.cfg] * self.K)[k]
        out = {"learning_rate": float(c.learning_rate), "clip_range": float(c.clip_range)}
        for fld, s in (self.hparam_schedules or {}).items():
            out[fld] = linear_schedule(out[fld], s["end"], s["end_fraction"], self.progress_remaining)
        return out

    def _store_scheduled_hparams(self) -> None:
        """a scheduled trainer's train() begins here (SB3: _update_learning_rate and clip_range(p), held for all epochs of the call): every
        replica's six hyper-parameters -- what the kernels otherwise get as scalars, ent_coef / world included -- into the handle's table,
        one eager launch, no host wait"""
        cfgs = getattr(self, "cfgs", None) or [self.cfg] * self.K
        self.scheduled_values = [self.scheduled_hparams(k) for k in range(self.K)]
        rows = []
        for c, now in zip(cfgs, self.scheduled_values):
            row = {f: float(getattr(c, f)) for f in self._mlp.HPARAM_FIELDS}
            row.update(now)
            row["ent_coef"] = c.ent_coef / self.dist.world_size
            rows.append(row)
        self._mlp.hparams_store(rows)

    def current_hparams(self, k: int = 0) -> dict[str, float]:
        """replica k's learning rate and clip range as the last train() call used them (SB3's train/learning_rate, train/clip_range; the
        optimiser group's lr): the config's constants without a schedule or before the first call"""
        c = (getattr(self, "cfgs", None) or [self.cfg] * self.K)[k]
        if self.hparam_schedules is not None and self.scheduled_values is not None:
            return dict(self.scheduled_values[k])
        return {"learning_rate": float(c.learning_rate), "clip_range": float(c.clip_range)}

    # ------------------------------------------------------------------ training monitor
    def _setup_monitor(self, monitor: bool | int) -> None:
        """``monitor=``: the device handle over the K x N rollout columns, the explained-variance output and the log_std snapshot.  The three
        kernels run once here, on the still zeroed buffers (no episode ends, the carries are cleared again), so that a rollout capture finds
        them loaded without the capture's warm-up step having to pass through them."""
        from . import monitor as _monitor

        window = _monitor.check_monitor(monitor, self.dist)
        self.monitor = None
        if not window:
            return
        T, K, N = self.cfg.n_steps, self.K, self.n_envs
        self.monitor = _monitor.EpisodeMonitor(self.device, K, N, window=window, max_steps=T)
        self._ev_dev = torch.zeros((K, 2), dtype=torch.float64, device=self.device)
        self._log_std_snap = torch.zeros((K, ACT_DIM), dtype=torch.float32, device=self.device)
        self.monitor.observe(self.rew_buf, self.done_buf, 1)
        self.monitor.reset_carry()
        self._monitor_explained_variance()

    def _monitor_observe(self) -> None:
        """first launch of the rollout tail: the episodes of this rollout, from the rewards as the env wrote them (before the time-limit
        bootstrap adds gamma * V into them).  The capture warm-up's tail does not feed it: its one step is rolled back."""
        if self.monitor is not None and self._monitor_live:
            self.monitor.observe(self.rew_buf, self.done_buf, self.cfg.n_steps)

    def _monitor_explained_variance(self) -> None:
        """last launch of the rollout tail: var(returns) and var(returns - values) per replica (SB3 train(): explained_variance of the rollout
        buffer's values and returns)"""
        if self.monitor is None:
            return
        T, KN = self.cfg.n_steps, self.K * self.n_envs
        native.check(self.L.kp1_explained_variance(native.device_index(self.device), native.ptr(self.val_buf), native.ptr(self.ret_buf), T, KN, self.n_envs,
                                                   native.ptr(self._ev_dev), native.stream_arg(self.device)))

    def monitor_rows(self) -> list[dict[str, Any]]:
        """SB3's rollout/ and train/ keys of the last iteration, one dict per replica (monitor.KEYS without the time/ keys, which a
        ``monitor.TrainLogger`` adds).  Reading it synchronises with the device, like ``last_stats``."""
        if self.monitor is None:
            raise RuntimeError("monitor_rows needs a trainer constructed with monitor=True (or a window size)")
        from . import monitor as _monitor

        ev = self._ev_dev.tolist()
        std = torch.exp(self._log_std_snap).mean(dim=1).tolist()     # th.exp(policy.log_std).mean(), in fp32 as SB3 takes it
        stats = self._stats_rows()
        rows = []
        for k in range(self.K):
            row = _monitor.episode_record(self.monitor.read(k))
            s = stats[k]
            now = self.current_hparams(k)      # under a schedule: the values the last train() used
            row.update({"train/approx_kl": s.get("approx_kl"), "train/clip_range": now["clip_range"],
                        "train/entropy_loss": -s["entropy"] if "entropy" in s else None,
                        "train/explained_variance": _monitor.explained_variance(ev[k][0], ev[k][1]),
                        "train/learning_rate": now["learning_rate"], "train/n_updates": self.n_updates(k),
                        "train/policy_gradient_loss": s.get("policy_loss"), "train/std": std[k] if self.n_train_calls else None,
                        "train/value_loss": s.get("value_loss")})
            if self.kl_targets is not None and self._kl_fresh[k]:     # reported once: TrainLogger prints SB3's early-stopping line
                row["kl_stop"] = {q: self._kl_records[k][q] for q in ("stop_epoch", "stop_minibatch", "stop_kl")}
                self._kl_fresh[k] = False
            rows.append(row)
        return rows

    def make_loggers(self, csv_paths: list[Any] | None = None) -> list[Any]:
        """one ``monitor.TrainLogger`` per replica, on this run's current step clock (``csv_paths[k]``: replica k's progress.csv or None)"""
        from . import monitor as _monitor

        paths = csv_paths if csv_paths is not None else [None] * self.K
        return [_monitor.TrainLogger(paths[k], start_timesteps=self.num_timesteps) for k in range(self.K)]

    def _sl(self, k: int) -> slice:
        """replica k's columns of the rollout buffers"""
        return slice(k * self.n_envs, (k + 1) * self.n_envs)

    # Minibatch shuffles.  At the benchmarked size (524288 samples) a sort-based torch.randperm is 0.16 ms of full-chip kernels, eight times per
    # iteration (2.5 %); drawing them on a side stream under the rollout only moved that time (the sort kernels fill the chip and the
    # rollout's launches queue behind them: rollout +1.3 ms for update -1.7 ms).  From PERM_CIPHER_MIN samples on, the permutation is a keyed
    # bijection evaluated per element (kp1_random_permutation: one elementwise launch); below it torch.randperm stays -- it is cheap there.
    PERM_CIPHER_MIN = 1 << 17

    def _draw_perm(self, k: int) -> None:
        """replica k's indices of one epoch's minibatches into self.perm[k]: a random permutation of [0, T N) on the device (SB3:
        np.random.permutation in RolloutBuffer.get)"""
        out = self.perm[k]
        total = out.numel()
        if total < self.PERM_CIPHER_MIN:
            torch.randperm(total, device=self.device, generator=self.gens[k], out=out)
            return
        keys = self._perm_rngs[k].integers(0, 1 << 32, size=8, dtype=np.uint64).astype(np.uint32)
        native.check(self.L.kp1_random_permutation(native.device_index(self.device), total, keys.ctypes.data_as(C.c_void_p), native.ptr(out),
                                                   native.stream_arg(self.device)))

    def _draw_noise(self) -> None:
        """the exploration noise of the whole rollout"""
        self.noise_all.normal_(generator=self.gens[0])

    def invalidate_graphs(self) -> None:
        """Drop the captured hipGraphs: a capture freezes host-side scalars into kernel arguments (env stage / mode / config pointers; learning
        rate, clip range, ent / vf coefficients, minibatch geometry), so after changing any of them the next rollout / epoch is re-captured.
        Called automatically when ``env.launch_args_version`` or the PPOConfig fields the epoch graph bakes in have changed."""
        self._rollout_graph = None
        self._epoch_graph = None

    def _epoch_key(self) -> tuple:
        c = self.cfg
        key = (c.learning_rate, c.clip_range, c.ent_coef, c.vf_coef, c.max_grad_norm, c.adam_eps, c.batch_size, c.n_steps, c.normalize_advantage,
               self.dist.world_size, self._mlp.train_tile)
        if self.hparam_schedules is not None:
            # a scheduled trainer's kernels read learning rate and clip range from the handle's table: the graph froze its address, so the key
            # carries which of the two are scheduled in place of the values
            key = key[2:-1] + (("hparam_line", tuple(sorted(self.hparam_schedules))),) + key[-1:]
        if self.kl_targets is not None:     # a gated trainer captured the gated launches; the last element stays the train-tile flag
            key = key[:-1] + (("kl_gate", tuple(self.kl_targets)),) + key[-1:]
        return key

    def _curriculum_observe(self, t: int) -> None:
        """after env step t: feed the done bytes to the device tracker (single process: every step; data parallel: once per chunk -- a route
        tracker gets the step's episode records, written every step, in place of the done bytes)"""
        cur = self._rollout_tracker()
        if cur is None:
            return
        if not self.dist.enabled:
            cur.observe(self.done_buf[t], self.n_envs)
            return
        c = self.done_chunk
        if self._record_stage is not None:
            self.curriculum.record(self.done_buf[t], self._record_stage[t % c])
        if (t + 1) % c == 0:
            src = self.done_buf[t + 1 - c:t + 1] if self._record_stage is None else self._record_stage
            self.dist.all_gather_into(self._done_gather, src)
            self.curriculum.observe_chunk(self._done_gather, self.n_envs, c, self.dist.world_size)

    # ------------------------------------------------------------------ PPO.load
    def load_checkpoint(self, path: str, *, restore_optimizer: bool = True, restore_timesteps: bool = False,
                        restore_hyperparameters: bool = False) -> dict[str, Any]:
        """``PPO.load(path, env=...)`` for an SB3 zip (the reference's resume paths, train_workspace_expansion.py:187-197,
        train_route_curriculum.py:129-139): policy weights, and the Adam state of ``policy.optimizer.pth`` when present -- first / second
        moments per tensor and torch's per-tensor step counts (a common count, plus the extra steps of the actor tensors when a
        teacher-anchor run wrote the file).  ``restore_hyperparameters``: a loaded SB3 model keeps the algorithm constants it was saved
        with (gamma, gae_lambda, ent_coef, vf_coef, max_grad_norm, n_epochs, normalize_advantage, and clip_range when the zip stores it
        as a plain value); the trainers then re-apply only the YAML's learning rate.  The rollout geometry (n_envs, n_steps, minibatch)
        stays the engine's: it is sized for the GPU, not for the 12-16 CPU envs a reference checkpoint was collected with.  Must be called
        before the first update (the constants are baked into the captured graphs).  Returns what was restored."""
        from . import checkpoint

        self.policy.load_state_dict(checkpoint.load_policy_state_dict(path))
        restored: dict[str, Any] = {"policy": True, "optimizer": False}
        opt = checkpoint.load_optimizer_state_dict(path) if restore_optimizer else None
        if opt and opt.get("state"):
            self.adam_t, self.actor_extra_steps = load_adam_state(opt, self.policy.spec, self.adam_m, self.adam_v)
            restored.update({"optimizer": True, "adam_steps": self.adam_t, "actor_extra_steps": self.actor_extra_steps})
        self._mlp.pack(self.policy.flat)
        self._mlp.set_step_count(self.adam_t)
        self._mlp.set_actor_extra_steps(self.actor_extra_steps)
        if restore_timesteps or restore_hyperparameters:
            data = checkpoint.load_data(path)
            if restore_timesteps:
                self.num_timesteps = int(data.get("num_timesteps", 0))
                restored["num_timesteps"] = self.num_timesteps
                saved_epochs = data.get("n_epochs")
                if isinstance(data.get("_n_updates"), int) and isinstance(saved_epochs, int) and saved_epochs > 0:
                    self.n_train_calls = int(data["_n_updates"]) // saved_epochs   # SB3: _n_updates += n_epochs per train() call
            if restore_hyperparameters:
                if self._epoch_graph is not None or self.adam_t != restored.get("adam_steps", self.adam_t):
                    raise RuntimeError("restore_hyperparameters must happen before the first update")
                restored["hyperparameters"] = restore_saved_hyperparameters(self.cfg, data)
        self._kl_after_load()
        return restored

    # ------------------------------------------------------------------ policy evaluation
    def _forward(self, obs: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """mean[n,7], value[n] for obs [n, 56 or 64]"""
        return self._mlp.mean_value(obs.contiguous())

    def predict(self, obs: torch.Tensor, deterministic: bool = True) -> torch.Tensor:
        """model.predict(obs, deterministic): mean (or a sample) clipped to the action space (eval_three_stage.py:25-27)."""
        with torch.no_grad():
            mean, _ = self._forward(obs)
            if not deterministic:
                mean = mean + torch.exp(self.policy.views["log_std"]) * torch.randn(mean.shape, device=mean.device, generator=self.gens[0])
            return mean.clamp(-1.0, 1.0)

    def predict_unclipped(self, obs: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            return self._forward(obs)[0]

    def _bootstrap_truncated(self, dense: bool = False) -> None:
        """SB3 collect_rollouts time-limit bootstrap: rewards[t, i] += gamma * V(terminal_observation) where step t of env i was
        truncated and not terminated.  ``dense`` = critic over all T * N terminal observations + kp1_bootstrap_truncated (kept as the
        reference for the compacted one)."""
        cfg = self.cfg
        T, N = cfg.n_steps, self.n_envs
        if not dense:
            # the value net runs on the _trunc_cap terminal observations of the index list instead of all T * N
            cap = self._trunc_cap
            trunc = (self.done_buf.view(-1) & 3) == 2
            idx = torch.nonzero_static(trunc, size=cap, fill_value=0).view(-1)
            valid = torch.arange(cap, device=self.device) < trunc.sum()
            sel = self.term_obs_buf.view(T * N, self.obs_w).index_select(0, idx)
            tv = torch.empty(cap, dtype=torch.float32, device=self.device)
            for s0 in range(0, cap, self._mlp.max_batch):
                e0 = min(s0 + self._mlp.max_batch, cap)
                self._mlp.forward(sel[s0:e0], value=tv[s0:e0])
            self.rew_buf.view(-1).index_add_(0, idx, torch.where(valid, cfg.gamma * tv, torch.zeros_like(tv)))
        else:
            _, tv = self._forward(self.term_obs_buf.view(T * N, self.obs_w))
            tv = tv.contiguous()
            native.check(self.L.kp1_bootstrap_truncated(native.device_index(self.device), native.ptr(self.rew_buf), native.ptr(tv),
                                                        native.ptr(self.done_buf), cfg.gamma, T * N, native.stream_arg(self.device)))

    # ------------------------------------------------------------------ rollout
    @torch.no_grad()
    def collect_rollouts(self) -> None:
        cfg = self.cfg
        T, N = cfg.n_steps, self.n_envs
        if self._needs_reset:
            self._reset_envs()
            self._needs_reset = False
        else:
            self.obs_buf[0].copy_(self.obs_buf[T])
        world = self.dist.world_size
        graph_rollout = self.use_graphs and self.step_callback is None
        self._draw_noise()
        if graph_rollout:
            key = (tuple(getattr(env, "launch_args_version", 0) for env in self.envs), tuple(cur is not None for cur in self.curricula),
                   cfg.gamma, cfg.gae_lambda, self._whole_rollout)   # what a capture freezes
            if self._rollout_graph is None or self._rollout_graph_key != key:
                self._capture_rollout()
                self._rollout_graph_key = key
            self._replay_checked("rollout", self._rollout_graph)
        if not graph_rollout and self._whole_rollout:
            self._rollout_whole()          # one launch per span of env steps (never with a step callback), as the captured rollout replays it
        else:
            for t in range(0 if not graph_rollout else T, T):
                self._rollout_step_hip(t)      # the launch sequence the captured rollout replays
                if self.step_callback is not None:
                    self.step_callback(self.done_buf[t])
        if not graph_rollout:
            self._kernels_warm = True
        self.num_timesteps += T * N * world
        if not graph_rollout:
            self._post_rollout()     # (the captured rollout ends with it)

    def _post_rollout(self) -> None:
        """what SB3's collect_rollouts does after the last env step: time-limit bootstrap, value of the last observation, GAE.  Static shapes
        and no host synchronisation, so the captured rollout graph carries it as its tail (a dozen small launches whose host latency
        was 0.5 ms per iteration)."""
        self._monitor_observe()
        self._bootstrap_truncated()
        last_v = torch.empty(self.K * self.n_envs, dtype=torch.float32, device=self.device)
        self._mlp.forward(self.obs_buf[self.cfg.n_steps], value=last_v)   # value net only
        self._gae_scan(last_v)
        self._monitor_explained_variance()

    def _gae_scan(self, last_v: torch.Tensor) -> None:
        """GAE runs per column: one launch covers every replica (a population with overrides reads each replica's gamma and lambda)"""
        cfg = self.cfg
        native.check(self.L.kp1_gae_scan(native.device_index(self.device), native.ptr(self.rew_buf), native.ptr(self.val_buf), native.ptr(self.done_buf),
                                         native.ptr(last_v), cfg.gamma, cfg.gae_lambda, native.ptr(self.adv_buf), native.ptr(self.ret_buf), cfg.n_steps,
                                         self.K * self.n_envs, native.stream_arg(self.device)))

    def _rollout_step_hip(self, t: int) -> None:
        # (running the tracker on a side stream under the next policy forward was measured: the fork / join inside the graph
        # cost more than the 4 us kernel it hid -- 7.4 ms vs 5.9 ms per 128-step rollout)
        self._policy_env_step(t)
        self._curriculum_observe(t)

    def _policy_env_step(self, t: int) -> None:
        env = self._rollout_env()
        if self._fused_route_step:
            # a route env: policy forward + sampling + base step + nearest scan + route step (auto-reset included, a population's in each
            # replica's window) in ONE launch
            self._mlp.forward_route_step(env, self.obs_buf[t], noise=self.noise_all[t], value=self.val_buf[t], action=self.act_buf[t],
                                         log_prob=self.logp_buf[t], next_obs=self.obs_buf[t + 1], reward=self.rew_buf[t], done=self.done_buf[t],
                                         terminal_obs=self.term_obs_buf[t])
        elif self._fused_env_step:
            # policy forward + sampling + env step (auto-reset included, a population's on each replica's own stage) in ONE launch: the
            # tile's policy workgroup steps its 32 envs itself
            self._mlp.forward_env_step(env, self.obs_buf[t], noise=self.noise_all[t], value=self.val_buf[t], action=self.act_buf[t],
                                       log_prob=self.logp_buf[t], next_obs=self.obs_buf[t + 1], reward=self.rew_buf[t], done=self.done_buf[t],
                                       terminal_obs=self.term_obs_buf[t])
        else:
            self._mlp.forward(self.obs_buf[t], noise=self.noise_all[t], value=self.val_buf[t], action=self.act_buf[t],
                              clipped=self.clip_act, log_prob=self.logp_buf[t])
            env.step_into(self.clip_act, self.obs_buf[t + 1], self.rew_buf[t], self.done_buf[t], self.term_obs_buf[t], True)

    def _capture_rollout(self) -> None:
        """Record the T-step rollout (policy forward, env step, curriculum tracker; data parallel: the done-byte all-gather of every chunk)
        once; every later rollout is one replay.  The kernels must have run once before a capture (code objects loaded, attributes set).  At
        the very start that is a warm-up step between a device snapshot of every env's state and its restore; a RE-capture in the middle of
        training (an env setter or a hyper-parameter changed, a step callback was removed) finds them warm from the rollouts already done.
        Either way the running episodes and random streams are untouched."""
        T = self.cfg.n_steps
        if not self._kernels_warm:
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):
                for env in self.envs:
                    env.use_current_stream()
                    if hasattr(env, "snapshot"):
                        env.snapshot()       # the warm-up step below must not move the episodes or the random streams
                if self._whole_rollout:
                    self._rollout_whole(1, tracked=False)     # (a bound env steps without its tracker: nothing observes this step)
                else:
                    self._policy_env_step(0)
                self._warm_curricula()
                self._monitor_live = False   # (the monitor's kernels ran at construction; this step is rolled back and is no episode data)
                try:
                    self._post_rollout()     # the graph's tail, once eagerly (its buffers are rewritten by the real rollout)
                finally:
                    self._monitor_live = True
                fresh = []
                for k, env in enumerate(self.envs):
                    env.use_current_stream()
                    if hasattr(env, "snapshot"):
                        env.restore()        # a captured rollout therefore continues exactly like an eager one (tests/test_distributed_gpu.py)
                    else:
                        # wrappers without a device snapshot (the route env keeps state of its own): start the episodes again instead, at
                        # the price of one extra reset() draw per env stream
                        fresh.append(k)
                if fresh:
                    self._reset_envs(fresh)
            torch.cuda.current_stream(self.device).wait_stream(side)
            self._kernels_warm = True
        torch.cuda.synchronize(self.device)

        whole = self._whole_rollout

        def body() -> None:
            if whole:
                self._rollout_whole()      # two launches per span: the env steps (tracker included), the critic
            else:
                for t in range(T):
                    self._rollout_step_hip(t)
            self._post_rollout()

        self._rollout_graph = self._capture(body, on_begin=self._envs_use_current_stream)
        self._envs_use_current_stream()

    def _reset_envs(self, which: list[int] | None = None) -> None:
        """obs_buf[0] <- reset() of the env handles `which` (default: all), each into its replica's columns"""
        for k in range(len(self.envs)) if which is None else which:
            self.obs_buf[0, self._sl(k)].copy_(self.envs[k].reset())
        self._monitor_reset_carry()

    def _monitor_reset_carry(self) -> None:
        """after an explicit env reset: the running episodes were abandoned, so their partial returns and lengths are dropped"""
        if self.monitor is not None:
            self.monitor.reset_carry()

    def _warm_curricula(self) -> None:
        """the capture warm-up's tracker launch: every tracker once on zeroed done bytes with a zero clock step (moves nothing; also loads
        the module the chunk form of the tracker lives in)"""
        for k, cur in enumerate(self.curricula):
            if cur is not None:
                cur.observe(self.done_buf[0, self._sl(k)].zero_(), 0)

    def _envs_use_current_stream(self) -> None:
        for env in self.envs:
            env.use_current_stream()

    def _capture(self, body, on_begin=None):
        """record `body` once: ONE hipGraph (single process, or collectives captured inside), or a GraphSegments chain cut at every collective"""
        if self.dist.enabled and self.graph_mode == "segmented":
            seg = GraphSegments(self.device, on_begin=on_begin)
            self.dist._segments = seg
            try:
                seg.begin()
                body()
                seg.finish()
            except BaseException:
                seg.abort()
                raise
            finally:
                self.dist._segments = None
            return seg
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local" if self.dist.enabled else "global"):
            if on_begin is not None:
                on_begin()
            body()
        return g

    def _replay_checked(self, what: str, graph) -> None:
        """replay; the FIRST replay of a graph that has RCCL collectives captured inside runs under a watchdog and is followed by a check
        that every rank still holds the same parameters (that path has no recorded multi-GPU run: a hang or a divergence must end the job
        with a message instead of a silent wrong result)"""
        if self._first_replay_checked[what]:
            graph.replay()
            return
        dog = self.dist.watchdog(300.0, f"the first replay of the {what} graph with captured RCCL collectives")
        graph.replay()
        torch.cuda.synchronize(self.device)
        ok = self.dist.ranks_agree(self.policy.flat)
        dog.cancel()
        self._first_replay_checked[what] = True
        if not ok:
            raise RuntimeError(f"ranks diverged after the first replay of the {what} graph with captured RCCL collectives; re-run with KP1_DIST_GRAPHS=0")

    # ------------------------------------------------------------------ update
    def train(self) -> None:
        cfg, n_mb = self.cfg, self._n_minibatches()
        gated = self.kl_targets is not None
        if gated:
            self._resolve_kl()      # the previous call's records, before arming clears them
        self.n_train_calls += 1
        self.stats_dev.zero_()
        if gated:
            self._mlp.kl_gate_arm()
        if self.hparam_schedules is not None:
            self._store_scheduled_hparams()
        for _epoch in range(cfg.n_epochs):
            for k in range(self.K):
                self._draw_perm(k)
            if gated and not self.use_graphs:
                self._epoch_body()     # the device's per-replica counts are the truth: the host mirror follows them (_resolve_kl)
            elif not self.use_graphs:
                # the eager epoch steps Adam from the device-resident step count too, exactly as the captured epoch does (bias corrections
                # computed by the same device arithmetic): eager and replayed training stay bit-identical.  The count is set from the host
                # mirror first, so loss_grad calls made outside train() cannot have moved it.
                self._mlp.set_step_count(self.adam_t)
                self._epoch_body()
            elif self._epoch_graph is None and not self._epoch_warm:
                self._epoch_warm = True      # one eager epoch first (warm-up + it is a real epoch), then capture for the following ones
                self._epoch_body()
            elif self._epoch_graph is None or self._epoch_graph_key != self._epoch_key():
                self._epoch_graph = None     # (a hyper-parameter baked into the captured kernel arguments changed: capture again)
                torch.cuda.synchronize(self.device)
                self._epoch_graph = self._capture(self._epoch_body)
                self._epoch_graph_key = self._epoch_key()
                self._epoch_auto = {"phase": 0} if (self.graph_mode == "segmented" and self._epoch_policy == "auto") else None
                self._replay_checked("epoch", self._epoch_graph)      # the first replay carries one-time costs: never the timed one
            else:
                if self.graph_mode == "segmented" and self._segmented_epoch_eager():
                    self._epoch_body()     # data parallel, segments measured slower than eager launches on this box (same bits either way)
                else:
                    self._replay_checked("epoch", self._epoch_graph)
                self._segmented_epoch_timed()
            if not gated:
                self.adam_t += n_mb
        # read back lazily (last_stats): a .tolist() here would make every iteration wait for its own update before the host can enqueue
        # the next rollout
        self._last_stats_dev = (self.stats_dev.clone(), n_mb * cfg.n_epochs)
        if gated:
            self._kl_pending = torch.cuda.Event()
            self._kl_pending.record(torch.cuda.current_stream(self.device))
        if self.monitor is not None:
            # train/std: exp(log_std) after the update; 7 floats per replica, device to device
            self._log_std_snap.copy_(self.flat.view(self.K, -1)[:, :ACT_DIM])

    def _epoch_body(self) -> None:
        """one update epoch from the shuffle in self.perm: advantage statistics of all minibatches (+ ONE all-reduce of them), then per
        minibatch tile kernel, weight gradients, finalize, [flat gradient all-reduce, sum of squares], Adam.  The epoch graph records it; the
        warm-up, segmented-eager and eager epochs call it directly."""
        cfg = self.cfg
        T = cfg.n_steps
        total = T * self.n_envs
        local_bs = max(cfg.batch_size // self.dist.world_size, 1)
        obs = self.obs_buf[:T].view(total, self.obs_w)
        act, old_logp = self.act_buf.view(total, ACT_DIM), self.logp_buf.view(total)
        adv, ret = self.adv_buf.view(total), self.ret_buf.view(total)
        perm = self.perm[0]
        mb_stats = self._epoch_adv_stats(adv, perm, total, local_bs)
        for i, start in enumerate(range(0, total, local_bs)):
            self._hip_minibatch_step(obs, perm[start:start + local_bs], act, old_logp, adv, ret, device_step=True,
                                     adv_stats=None if mb_stats is None else mb_stats[i])

    # Data parallel, graph_mode "segmented": an update epoch is 64 graph segments of four kernels with a collective between them.  A hipGraph
    # launch boundary costs more on the GPU timeline than a kernel boundary of an eager launch (one-rank RCCL group on one MI355X, collectives
    # stubbed out: 48.9 ms per update as segments, 45.6 ms as eager launches, 43.7 ms as ONE graph without a process group), while a slow or
    # busy host favours the segments.  Both forms leave the same bits (tests/test_distributed_gpu.py), so the choice is measured: after the
    # capture, one replayed epoch and one eager epoch are timed with events, the times are max-reduced over the ranks, and the faster form
    # runs from then on (KP1_DP_EPOCH=graph|eager pins it).
    def _segmented_epoch_eager(self) -> bool:
        if self._epoch_policy != "auto":
            return self._epoch_policy == "eager"
        a = self._epoch_auto
        if a is None:
            return False
        if a["phase"] in (0, 1):          # phase 0: time a replay; phase 1: time an eager epoch
            a["ev"] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            a["ev"][0].record()
            return a["phase"] == 1
        return bool(a["eager"])

    def _segmented_epoch_timed(self) -> None:
        a = self._epoch_auto
        if a is None or self._epoch_policy != "auto" or a["phase"] > 1:
            return
        a["ev"][1].record()
        a["t_graph" if a["phase"] == 0 else "t_eager"] = a["ev"]
        a["phase"] += 1
        if a["phase"] == 2:
            torch.cuda.synchronize(self.device)
            t = torch.tensor([a["t_graph"][0].elapsed_time(a["t_graph"][1]), a["t_eager"][0].elapsed_time(a["t_eager"][1])], dtype=torch.float64, device=self.device)
            if self.dist.enabled:
                self.dist.dist.all_reduce(t, op=self.dist.dist.ReduceOp.MAX)      # every rank takes the same form
            a["ms"] = [float(x) for x in t.tolist()]
            a["eager"] = a["ms"][1] < a["ms"][0]
            self.epoch_form = "eager launches" if a["eager"] else "graph segments"

    @property
    def last_stats(self) -> dict[str, float]:
        """mean policy loss / value loss / entropy / approx_kl over the minibatches of the last train() call, and their number (SB3 logger keys
        train/policy_gradient_loss, train/value_loss, train/entropy_loss, train/approx_kl); reading it synchronises with that update"""
        return self._stats_rows()[0]

    def _stats_rows(self) -> list[dict[str, float]]:
        """last_stats of every replica"""
        if self._last_stats_dev is not None:
            stats, n_updates = self._last_stats_dev
            names = ("policy_loss", "value_loss", "entropy", "approx_kl")
            if self.kl_targets is None:
                rows = (stats / max(n_updates, 1)).tolist()
                self._last_stats_host = [dict(zip(names, r), n_updates=n_updates) for r in rows]
            else:     # the means are over the minibatches that entered the statistics: up to and including the one that stopped
                self._resolve_kl()
                counts = [r["n_counted"] for r in self._kl_records]
                div = torch.tensor([max(c, 1) for c in counts], dtype=torch.float32, device=stats.device).view(-1, 1)
                rows = (stats / div).tolist()
                self._last_stats_host = [dict(zip(names, r), n_updates=c, **{q: v for q, v in rec.items() if q != "n_counted"})
                                         for r, c, rec in zip(rows, counts, self._kl_records)]
            self._last_stats_dev = None
        return self._last_stats_host

    def _epoch_adv_stats(self, adv, perm, total: int, local_bs: int):
        """(mean, 1/(std + 1e-8)) of the advantages of every minibatch of this epoch, on the device: f32 [n_minibatches, 2] for one shuffle
        ``perm`` [total]; [n_minibatches][K][2] for a population's [K, total] block of shuffles, each row summed by a launch of its own.

        SB3 normalises per minibatch (ppo.py train()).  One kernel sums all minibatches, and with data parallelism ONE
        all-reduce per epoch makes the statistics those of the global minibatch (all ranks' shards together), so the
        update does not depend on how the rollout is sharded -- instead of a 3-float collective before every optimiser step."""
        if not self.cfg.normalize_advantage:
            return None
        n_mb = (total + local_bs - 1) // local_bs
        one = perm.dim() == 1
        lead = (n_mb,) if one else (perm.shape[0], n_mb)
        sums = torch.empty((*lead, 3), dtype=torch.float64, device=self.device)
        dev, stream = native.device_index(self.device), native.stream_arg(self.device)
        rows = [(perm, sums)] if one else [(perm[k], sums[k]) for k in range(perm.shape[0])]
        for row, out in rows:
            native.check(self.L.kp1_adv_minibatch_sums(dev, native.ptr(adv), native.ptr(row), total, local_bs, native.ptr(out), stream))
        self.dist.all_reduce_sum(sums)
        stats = torch.empty((*lead, 2), dtype=torch.float32, device=self.device)
        native.check(self.L.kp1_adv_minibatch_stats(dev, native.ptr(sums), sums.numel() // 3, native.ptr(stats), stream))
        return stats if one else stats.permute(1, 0, 2).contiguous()

    def _hip_minibatch_step(self, obs, idx, act, old_logp, adv, ret, device_step: bool = False, adv_stats=None) -> None:
        """THE optimiser step, all on the device: gathered fwd + loss + bwd (MFMA), flat grad all-reduce, clip + Adam + repack.  ``idx``: [n] rows,
        or a population's [K][n] block (with overrides the kernels read each replica's constants from the handle's table, not these scalars)"""
        cfg = self.cfg
        n = int(idx.numel()) // self.K
        world = self.dist.world_size
        if adv_stats is None and cfg.normalize_advantage and self.dist.enabled:
            mean, inv_std = global_advantage_stats(adv[idx], self.dist)
            adv_stats = torch.stack([mean, inv_std]).float()
        self._mlp.loss_grad(obs, idx, n, act, old_logp, adv, ret, clip_range=cfg.clip_range, ent_coef=cfg.ent_coef / world, vf_coef=cfg.vf_coef,
                            inv_count=1.0 / (n * world), grad_out=self.grad, stats_out=self.stats_dev, adv_stats=adv_stats,
                            normalize=cfg.normalize_advantage)
        self.dist.all_reduce_sum(self.grad)
        if not device_step:
            self.adam_t += 1
        # device_step: the Adam step count lives on the device (incremented by loss_grad's finalize kernel) so that the
        # launch sequence can be replayed from a hipGraph; the host mirror self.adam_t is advanced by the caller
        self._mlp.adam_step(self.flat, self.grad, self.adam_m, self.adam_v, lr=cfg.learning_rate, eps=cfg.adam_eps,
                            max_grad_norm=cfg.max_grad_norm, step=0 if device_step else self.adam_t, fused_norm=not self.dist.enabled)

    # ------------------------------------------------------------------ driver
    def learn(self, total_timesteps: int | None = None, log_every: int = 0) -> "PPO":
        """``total_timesteps`` and the logged steps / fps count each replica's own env steps"""
        run_training(self, int(total_timesteps if total_timesteps is not None else self.cfg.total_timesteps), log_every=log_every, status=status_line)
        return self


def run_training(trainer: PPO, total_timesteps: int, *, after_rollout=None, after_update=None, log_every: int = 0, status=None,
                 csv_paths: list[Any] | None = None, tag: str | None = None) -> tuple[float, int]:
    """THE training loop of every trainer (PPO.learn, the three CLIs and their --seeds forms): iterations of rollout and update until
    ``trainer`` (a PPO or any population; the step clock counts each replica's own env steps) has taken ``total_timesteps`` env steps from
    where its clock stands.  Per iteration: ``collect_rollouts()``, ``after_rollout(trainer)`` (the teacher anchor), SB3's
    ``_update_current_progress_remaining`` (``trainer.progress_remaining = 1 - num_timesteps / (start + total_timesteps)``, ``start`` the
    clock as the loop found it: what ``learn(reset_num_timesteps=False)`` computes; the schedules of ``train()`` read it), ``train()``,
    ``after_update(trainer, steps_taken)`` (gates, periodic checkpoints); then every ``log_every`` iterations (0: never) either the
    monitor's record per replica -- SB3's table, a row of ``csv_paths[k]`` where given, and under the line ``[tag] it=.. replica <name>``
    where a population's caller passes ``tag`` -- or, without a monitor and on rank 0, the line ``status(trainer, it, steps_taken,
    elapsed_seconds)``.  The loggers start here, on the clock as the loop finds it.  Returns (wall seconds after a device synchronise, env
    steps taken)."""
    t0 = time.time()
    start, it = trainer.num_timesteps, 0
    loggers = trainer.make_loggers(csv_paths) if trainer.monitor is not None else None
    while trainer.num_timesteps - start < total_timesteps:
        trainer.collect_rollouts()
        if after_rollout is not None:
            after_rollout(trainer)
        trainer.progress_remaining = 1.0 - float(trainer.num_timesteps) / float(start + total_timesteps)
        trainer.train()
        it += 1
        if after_update is not None:
            after_update(trainer, trainer.num_timesteps - start)
        if not log_every or it % log_every:
            continue
        if loggers is not None:
            for k, row in enumerate(trainer.monitor_rows()):
                if tag is not None:
                    print(f"[{tag}] it={it} replica {trainer.replica_names[k]}", flush=True)
                loggers[k].log(row, iteration=it, total_timesteps=trainer.num_timesteps)
        elif status is not None and trainer.dist.rank == 0:
            print(status(trainer, it, trainer.num_timesteps - start, time.time() - t0), flush=True)
    torch.cuda.synchronize(trainer.device)
    return time.time() - t0, trainer.num_timesteps - start


def status_line(ppo: PPO, it: int, steps: int, elapsed: float) -> str:
    """PPO.learn's and train.py's line at the logging cadence (a population through learn(): the stages and statistics as lists)"""
    stages = [cur.read().stage_index if cur is not None else -1 for cur in ppo.curricula]
    stats = ppo._stats_rows()
    return (f"[ppo] it={it} steps={ppo.num_timesteps} fps={steps / elapsed:,.0f} stage={stages[0] if ppo.K == 1 else stages} "
            f"rew={ppo.rew_buf.mean().item():.4f} {stats[0] if ppo.K == 1 else stats}")


class InferencePolicy:
    """``PPO.load(path)`` + ``model.predict(obs, deterministic=True)`` for evaluators and the demo loaders
    (eval_deterministic.py:66-79, eval_three_stage.py:25-27): mean action clipped to the action space."""

    def __init__(self, state_dict: dict[str, torch.Tensor], device: torch.device | int = 0, max_batch: int = 8192) -> None:
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        hidden, obs_dim = (int(v) for v in state_dict["mlp_extractor.policy_net.0.weight"].shape)
        self.obs_dim = obs_dim
        self.policy = ActorCritic(hidden, self.device, obs_dim=obs_dim)
        self.policy.load_state_dict(state_dict)
        from . import mlp as _mlp

        # 2x64 (SB3's default, what reference-trained archives hold), 2x128 and 2x256 all evaluate on the MFMA kernels; any other width is
        # refused by kp1_mlp_create_ex -- there is no torch fallback in the product path
        self._mlp = _mlp.MlpKernels(hidden, self.device, max_batch=max_batch, obs_dim=obs_dim)
        self._mlp.pack(self.policy.flat)

    @classmethod
    def load(cls, path: str, device: torch.device | int = 0, max_batch: int = 8192) -> "InferencePolicy":
        from . import checkpoint

        return cls(checkpoint.load_policy_state_dict(path), device=device, max_batch=max_batch)

    @torch.no_grad()
    def predict(self, obs: torch.Tensor, deterministic: bool = True) -> torch.Tensor:
        if not deterministic:
            raise NotImplementedError("evaluators use deterministic=True")
        mean, _ = self._mlp.mean_value(obs.contiguous())
        return mean.clamp(-1.0, 1.0)

    __call__ = predict


def ppo_loss_and_grad_torch(flat: torch.Tensor, spec, obs, act, old_logp, adv, ret, *, clip_range: float, ent_coef: float, vf_coef: float,
                            world_size: int = 1) -> torch.Tensor:
    """SB3's PPO loss on plain torch (any device), gradient w.r.t. the flat parameter vector, scaled so that summing the
    result over ``world_size`` equal shards gives the single-process gradient.  Used by the CPU/gloo data-parallel tests."""
    flat = flat.detach().clone().requires_grad_(True)
    P, off = {}, 0
    for name, shape in spec:
        n = math.prod(shape)
        P[name] = flat[off:off + n].view(shape)
        off += n
    mean, value = mlp_forward(P, obs)
    logp = gaussian_log_prob(act, mean, P["log_std"])
    ratio = torch.exp(logp - old_logp)
    denom = float(obs.shape[0] * world_size)
    pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).sum() / denom
    vl = ((ret - value) ** 2).sum() / denom
    ent = (0.5 + LOG_SQRT_2PI + P["log_std"]).sum()
    loss = pl + vf_coef * vl - ent_coef * ent / world_size
    (grad,) = torch.autograd.grad(loss, flat)
    return grad


def global_advantage_stats(adv: torch.Tensor, dist: "Dist") -> tuple[torch.Tensor, torch.Tensor]:
    """(mean, 1/(std + 1e-8)) of the advantages of ALL ranks (unbiased std), via one all-reduce of (sum, sum^2, count):
    makes the normalisation, and hence the update, independent of how the minibatch is sharded over GPUs."""
    s = torch.stack([adv.sum(), (adv * adv).sum(), torch.tensor(float(adv.numel()), device=adv.device, dtype=adv.dtype)])
    dist.all_reduce_sum(s)
    mean = s[0] / s[2]
    var = ((s[1] - s[2] * mean * mean) / (s[2] - 1.0)).clamp_min(0)
    return mean, 1.0 / (var.sqrt() + 1e-8)


def smoke() -> dict[str, Any]:
    """tiny rollout + update on cuda:0 for __graft_entry__.smoke()"""
    cfg_dict = kcfg.load_workspace_expansion_config(kcfg.builtin_config_dir() / "workspace_expansion_bigtrain.yaml")
    env_cfg = kcfg.to_env_config(cfg_dict)
    env = ArmKinematicVecEnv(env_cfg, 256, seed=806)
    env.set_curriculum_stage(5)
    ppo = PPO(env, PPOConfig(n_steps=16, batch_size=1024, n_epochs=2, hidden=256, learning_rate=6e-6, gamma=0.995, clip_range=0.1, ent_coef=3e-4, seed=806))
    before = ppo.policy.flat.clone()
    ppo.collect_rollouts()
    ppo.train()
    torch.cuda.synchronize()
    delta = (ppo.policy.flat - before).abs().max().item()
    assert math.isfinite(delta) and delta > 0.0, "PPO update did not change the parameters"
    assert torch.isfinite(ppo.adv_buf).all()
    env.close()
    return {"ppo_param_delta": delta, "ppo_backend": ppo.backend}
