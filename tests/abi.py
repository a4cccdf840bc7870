"""What the ABI tests read out of the API headers, with a text split of their own -- deliberately not rl_brain_trainer_amd.native's parser, which
is what those tests check.  A plain module: ``import abi``."""
from __future__ import annotations

import re

from rl_brain_trainer_amd import config as kcfg

HEADERS = ("kp1.h", "kp1_ppo.h", "kp1_route.h")


def header(name: str) -> str:
    """include/<name> without its comments"""
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", (kcfg.repo_root() / "include" / name).read_text(), flags=re.S)


def params(func: str, header_name: str | None = None) -> list[str]:
    """the parameter texts of ``func``'s prototype, split at the commas (``[]`` for ``(void)``); ``header_name`` None searches all three"""
    for name in (header_name,) if header_name else HEADERS:
        m = re.search(rf"\b{func}\s*\(([^)]*)\)\s*;", header(name))
        if m:
            return [p.strip() for p in m.group(1).split(",") if p.strip() not in ("", "void")]
    raise AssertionError(f"{func} is not declared in include/{header_name or '{' + ', '.join(HEADERS) + '}'}")


def prototypes() -> dict[str, tuple[str, list[str]]]:
    """{function: (return type text, parameter texts)} of every kp1_* function the three headers declare"""
    out = {}
    for name in HEADERS:
        for ret, func in re.findall(r"^[ \t]*([A-Za-z_][\w \t]*?[\s*]+)(kp1_\w+)\s*\([^)]*\)\s*;", header(name), flags=re.M):
            out[func] = (" ".join(ret.replace("*", " * ").split()), params(func, name))
    return out
