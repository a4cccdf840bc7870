"""Data-parallel route curriculum, the parts a CPU can check: the two new C entry points are exported and declared, the record bits do not
overlap the done bits, and the route trainer's command line still takes every flag it took before."""
from __future__ import annotations

import re

from conftest import ROOT
from rl_brain_trainer_amd import native

NEW_SYMBOLS = ("kp1_route_episode_records", "kp1_route_curriculum_observe_chunk")


def _header(name: str) -> str:
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S)


def test_library_exports_the_route_exchange_entry_points():
    L = native.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in native.declared_symbols(), name


def test_record_bits_are_disjoint_from_the_done_bits():
    route_h, kp1_h = _header("kp1_route.h"), _header("kp1.h")
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint\s+{name}\s*\(", route_h), name
    rec = {k: int(v) for k, v in re.findall(r"#define\s+KP1_ROUTE_REC_(READY|ORI_HIT|REGRESSION)\s+(\d+)", route_h)}
    assert set(rec) == {"READY", "ORI_HIT", "REGRESSION"}
    done = {k: int(v) for k, v in re.findall(r"KP1_DONE_([A-Z]+)\s*=\s*(\d+)", kp1_h)}
    assert set(done) >= {"TERMINATED", "TRUNCATED", "SUCCESS"}
    bits = list(rec.values()) + list(done.values())
    assert all(b > 0 and b & (b - 1) == 0 for b in bits), bits           # one bit each
    assert len(set(bits)) == len(bits)                                    # pairwise disjoint
    assert all(v < 16 for v in done.values()) and all(16 <= v < 256 for v in rec.values())   # done bits 0-3, flags above, one byte


def test_train_route_parser_keeps_its_flags():
    from rl_brain_trainer_amd import train_route

    args = train_route.build_arg_parser().parse_args(
        ["--config", "c.yaml", "--route-path", "r.json", "--init-checkpoint", "m.zip", "--run-id", "x", "--output-dir", "o", "--total-timesteps", "100",
         "--seed", "3", "--n-envs", "64", "--n-steps", "16", "--batch-size", "512", "--hidden", "128", "--device", "0", "--log-every", "2"])
    assert (args.config, args.route_path, args.init_checkpoint, args.run_id, args.output_dir) == ("c.yaml", "r.json", "m.zip", "x", "o")
    assert (args.total_timesteps, args.seed, args.n_envs, args.n_steps, args.batch_size, args.hidden, args.device, args.log_every) == (100, 3, 64, 16, 512, 128, 0, 2)
