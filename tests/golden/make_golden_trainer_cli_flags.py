#!/usr/bin/env python3
"""Every flag of the three trainer entry points as argparse holds it (trainer_cli_flags.json): the record tests/test_trainer_cli_cpu.py
rebuilds from today's parsers and compares for equality.  The committed file was written from the parsers as they stood before the shared
CLI layer (trainer_cli.add_shared_flags) existed; regenerate it only when a flag changes on purpose.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_trainer_cli_flags.py
"""
from __future__ import annotations

import importlib
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent
MODULES = ("train", "train_dock", "train_route")


def parser_record(parser) -> dict:
    """{first option string: what argparse keeps of the action}; ``exclusive_with`` = the options of its mutually exclusive group"""
    group_of = {id(a): sorted(o for b in g._group_actions for o in b.option_strings) for g in parser._mutually_exclusive_groups for a in g._group_actions}
    return {(a.option_strings or [a.dest])[0]: {
        "option_strings": list(a.option_strings), "dest": a.dest, "default": a.default, "const": a.const,
        "type": getattr(a.type, "__name__", None) if a.type is not None else None, "choices": list(a.choices) if a.choices is not None else None,
        "required": a.required, "metavar": a.metavar, "help": a.help, "action": type(a).__name__, "exclusive_with": group_of.get(id(a)),
    } for a in parser._actions}


def records() -> dict:
    return {m: parser_record(importlib.import_module(f"rl_brain_trainer_amd.{m}").build_arg_parser()) for m in MODULES}


if __name__ == "__main__":
    sys.path.insert(0, str(OUT.parents[1]))
    (OUT / "trainer_cli_flags.json").write_text(json.dumps(records(), indent=1, sort_keys=True) + "\n")
