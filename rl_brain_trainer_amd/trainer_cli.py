"""What the trainer entry points (train, train_dock, train_route) share besides the loop itself (ppo.run_training): the flags all three
take, the switches those flags throw, the process context (device and process group) and two artefact helpers.  A flag, a refusal or an
export that every trainer has is written here once; what one trainer alone has stays in its file.
"""
from __future__ import annotations

import contextlib
import json
import os
import types
from pathlib import Path
from typing import Any

import torch

from . import monitor as _monitor


def add_shared_flags(parser, *, artifact_flag: str, sweep_under: str = "", log_every: int = 1, train_tile_group=None) -> None:
    """--seed / --seeds, --sweep, --hidden, --log-every, --train-tile and the monitor's two flags.  ``artifact_flag``: how the parser's
    help calls its artefact directory (<artifact-root>, <output-dir>); ``sweep_under``: what --sweep's help puts before the replica
    directory; ``log_every``: the trainer's default cadence; ``train_tile_group``: the mutually exclusive group --train-tile joins."""
    seeds = parser.add_mutually_exclusive_group()
    seeds.add_argument("--seed", type=int)
    seeds.add_argument("--seeds", help="comma-separated seeds trained together as one population (2x64 / 2x128 nets, one GPU); seed s writes "
                                       f"the artefacts of a --seed s run under {artifact_flag}/seed_<s>/, plus population_summary.json")
    parser.add_argument("--sweep", action="append", metavar="KEY=v1,v2", help="with --seeds: train every seed with each value of a PPO hyper-parameter "
                        "(repeatable; replicas = seeds x values, seed-major, at most 16); each replica writes what --seed s with those settings writes "
                        f"under {sweep_under}seed_<s>_<key>_<value>/")
    parser.add_argument("--hidden", type=int, default=256)
    parser.add_argument("--log-every", type=int, default=log_every)
    (train_tile_group or parser).add_argument(
        "--train-tile", dest="train_tile", action="store_true",
        help="hidden 64 / 128: forward, loss and backward of the optimiser step in one tile launch (train_tile128_kernel; sets "
             "KP1_TRAIN_TILE=1); without the flag KP1_TRAIN_TILE decides, and unset it is the layer-wise kernels")
    _monitor.add_cli_flags(parser)


def apply_switches(args) -> None:
    """what the parsed flags decide before anything else runs: --sweep without --seeds is refused, and the flags that stand for an
    environment variable export it (each where the parser has the flag)"""
    if args.sweep and args.seeds is None:
        raise ValueError("--sweep needs --seeds: a sweep trains its settings together as one population")
    if getattr(args, "train_tile", False):
        os.environ["KP1_TRAIN_TILE"] = "1"     # read by PPO._setup (every trainer class) when it creates the MLP handle
    if getattr(args, "whole_rollout", None) is not None:
        os.environ["KP1_ROLLOUT_RUN"] = "1" if args.whole_rollout else "0"     # read by PPO / ApproachPopulationPPO at every rollout
    if getattr(args, "one_launch_rollout", False):
        os.environ["KP1_FUSED_ROUTE_ROLLOUT"] = "1"     # read by PPO / RoutePopulationPPO at every rollout step (ppo.fused_route_rollout_covered)


@contextlib.contextmanager
def process_context(args):
    """The process a trainer runs in: ``world`` / ``rank`` of the process group the caller already initialised, else WORLD_SIZE / RANK as
    torchrun sets them; ``device`` = LOCAL_RANK, else the parser's --device where it has one, else 0 (made current); for world > 1 without
    a group, an nccl group of its own (``own_group``).  The body sets ``trainer`` once it has one: leaving without an error, the ranks of
    a data-parallel trainer meet at a barrier (the others wait for rank 0's evaluation and artefacts) and its launch-stream communicator
    is closed; a group made here is destroyed however the body ends."""
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        world, rank = dist.get_world_size(), dist.get_rank()
    else:
        world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    device = int(os.environ["LOCAL_RANK"]) if "LOCAL_RANK" in os.environ else int(getattr(args, "device", 0))
    torch.cuda.set_device(device)
    proc = types.SimpleNamespace(world=world, rank=rank, device=device, own_group=False, trainer=None)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device))
        proc.own_group = True
    try:
        yield proc
        if proc.trainer is not None and proc.trainer.dist.enabled:
            dist.barrier()
            proc.trainer.dist.close()
    finally:
        if proc.own_group:
            dist.destroy_process_group()


def refuse_population_under_dp(world: int) -> None:
    if world > 1:
        raise ValueError("--seeds trains a population on one GPU; it does not combine with data parallel")


def replica_extra(seed: int, name: str, overrides_k: dict[str, float] | None) -> dict[str, Any]:
    """what training_summary.json of a population replica holds on top of a --seed run's (``overrides_k``: None without --sweep)"""
    return {"seed": seed} if overrides_k is None else {"seed": seed, "replica": name, "overrides": dict(overrides_k)}


def write_json(path: Path, payload: dict[str, Any], **dumps: Any) -> None:
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(payload, indent=2, **dumps))
