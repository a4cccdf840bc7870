"""The whole-episode evaluation kernel without a GPU: kp1_eval_episodes is exported, declared and bound with matching argument lists; the
NULL and step-range refusals (made before any handle is looked at); the ``whole_episodes`` keyword and its defaults table on fakes; the flags
of both trainers."""
from __future__ import annotations

import ctypes as C
import inspect
import re
import types

import pytest

import abi
from rl_brain_trainer_amd import evaluate as ev
from rl_brain_trainer_amd import native, train, train_dock
from rl_brain_trainer_amd import workspace_coverage as wc

CTYPES = {"kp1_mlp*": C.c_void_p, "kp1_env*": C.c_void_p, "float*": C.c_void_p, "uint8_t*": C.c_void_p, "const double*": C.c_void_p, "void*": C.c_void_p,
          "int32_t": C.c_int32}


def test_symbol_is_exported_declared_and_bound_as_the_header_says():
    L = native.load()
    assert hasattr(C.CDLL(str(native.LIB_PATH)), "kp1_eval_episodes")
    assert "kp1_eval_episodes" in native.declared_symbols()
    header = abi.header("kp1_ppo.h")
    params = abi.params("kp1_eval_episodes", "kp1_ppo.h")
    assert len(params) == len(L.kp1_eval_episodes.argtypes) == 11
    for text, ctype in zip(params, L.kp1_eval_episodes.argtypes):
        decl = text.rsplit(None, 1)[0]                     # drop the parameter name
        if decl == "const kp1_eval_buffers*":
            assert ctype is C.POINTER(native.EvalBuffers), text
        else:
            assert CTYPES[decl] is ctype, text
    assert int(re.search(r"#define\s+KP1_EVAL_EPISODES_MAX_STEPS\s+(\d+)", header).group(1)) == native.EVAL_EPISODES_MAX_STEPS == ev._EPISODES_CAP == 256


def _last_error() -> str:
    L = native.load()
    L.kp1_last_error.restype = C.c_char_p
    return L.kp1_last_error().decode()


def test_null_and_range_refusals_need_no_device():
    """the refusals that come before a handle is dereferenced: a fake non-NULL pointer stands for every handle and array"""
    L = native.load()
    scratch = (C.c_char * 64)()
    p = C.cast(scratch, C.c_void_p)
    full = native.EvalBuffers(*[p.value] * 9)
    assert L.kp1_eval_episodes(None, None, None, None, None, None, 1, 4, None, 0, None) == -1
    assert "NULL argument to kp1_eval_step" in _last_error()
    for slot in range(5):
        args = [p, p, p, p, p]
        args[slot] = None
        assert L.kp1_eval_episodes(*args, C.byref(full), 1, 4, None, 0, None) == -1 and "NULL argument" in _last_error()
    for field in ("metrics", "counters", "flags", "state", "n_alive"):
        part = native.EvalBuffers(*[p.value] * 9)
        setattr(part, field, None)
        assert L.kp1_eval_episodes(p, p, p, p, p, C.byref(part), 1, 4, None, 0, None) == -1 and "kp1_eval_step: NULL buffer" in _last_error()
    part = native.EvalBuffers(*[p.value] * 9)
    part.hand_state = None
    assert L.kp1_eval_episodes(p, p, p, p, p, C.byref(part), 1, 4, None, 0, None) == -1 and "incomplete handoff buffers" in _last_error()
    for first, last, text in ((0, 4, "first_step must be at least 1"), (-3, -1, "first_step must be at least 1"), (5, 4, "last_step is below first_step"),
                              (1, 257, "at most KP1_EVAL_EPISODES_MAX_STEPS (256)"), (10, 2**31 - 1, "at most KP1_EVAL_EPISODES_MAX_STEPS (256)")):
        assert L.kp1_eval_episodes(p, p, p, p, p, C.byref(full), first, last, None, 0, None) == -1, (first, last)
        assert text in _last_error(), (first, last, _last_error())
    # kp1_eval_step keeps its own text for its step
    assert L.kp1_eval_step(p, p, p, p, p, C.byref(full), 0, None, 0, None) == -1 and "kp1_eval_step accounts env steps 1, 2, ..." in _last_error()


ENTRY_POINTS = {"evaluate_workspace_expansion": ev.evaluate_workspace_expansion, "run_pairs": wc.run_pairs,
                "evaluate_workspace_expansion_population": ev.evaluate_workspace_expansion_population, "evaluate_dock": train_dock.evaluate_dock}


def test_keyword_and_defaults_table():
    assert set(ev.WHOLE_EPISODES_DEFAULT) == set(ENTRY_POINTS) and all(type(v) is bool for v in ev.WHOLE_EPISODES_DEFAULT.values())
    for fn in (*ENTRY_POINTS.values(), wc._run_pairs_columns, wc.evaluate_full_workspace_coverage):
        q = inspect.signature(fn).parameters["whole_episodes"]
        assert q.default is None and q.kind in (inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD), fn
    q = inspect.signature(ev.run_episodes_fused).parameters["whole_episodes"]
    assert q.default is False and q.kind is inspect.Parameter.KEYWORD_ONLY
    for entry, default in ev.WHOLE_EPISODES_DEFAULT.items():
        assert ev.whole_episodes_default(entry, None) is default
        assert ev.whole_episodes_default(entry, True) is True and ev.whole_episodes_default(entry, False) is False


class _Policy:
    def __init__(self, mlp):
        self._mlp = mlp

    def predict(self, obs, deterministic=True):
        return obs


def test_run_phase_resolves_the_keyword_on_fakes(monkeypatch):
    """covered phase: run_episodes_fused gets the explicit value, or the entry point's default; uncovered phase: True raises, None and False
    take run_episodes"""
    seen = []
    monkeypatch.setattr(ev, "run_episodes_fused", lambda env, mlp, opts, **kw: seen.append(("fused", kw["whole_episodes"])))
    monkeypatch.setattr(ev, "run_episodes", lambda env, policy, opts, **kw: seen.append(("plain", kw)))
    mlp = types.SimpleNamespace(hidden=256, obs_dim=56, replicas=1, fused=True)
    monkeypatch.setattr(ev, "_one_launch_mlp", lambda policy, env, one_launch, what: None if one_launch is False or policy is None else mlp)
    pol = _Policy(mlp)
    for table_value in (False, True):
        monkeypatch.setitem(ev.WHOLE_EPISODES_DEFAULT, "run_pairs", table_value)
        seen.clear()
        ev.run_phase(object(), pol, {}, one_launch=None, what="Approach", whole_episodes=None, entry="run_pairs")
        ev.run_phase(object(), pol, {}, one_launch=None, what="Approach", whole_episodes=True, entry="run_pairs")
        ev.run_phase(object(), pol, {}, one_launch=None, what="Approach", whole_episodes=False, entry="run_pairs")
        ev.run_phase(object(), pol, {}, one_launch=None, what="Approach")
        assert seen == [("fused", table_value), ("fused", True), ("fused", False), ("fused", False)]
        seen.clear()
        ev.run_phase(object(), None, {}, one_launch=None, what="Approach", whole_episodes=None, entry="run_pairs")      # not covered: the default never raises
        ev.run_phase(object(), pol, {}, one_launch=False, what="Approach", whole_episodes=False, entry="run_pairs")
        assert seen == [("plain", {}), ("plain", {})]
        with pytest.raises(ValueError, match="whole_episodes=True: the Finisher phase is not covered"):
            ev.run_phase(object(), None, {}, one_launch=None, what="Finisher", whole_episodes=True, entry="run_pairs")
        with pytest.raises(ValueError, match="whole_episodes=True"):
            ev.run_phase(object(), pol, {}, one_launch=False, what="Approach", whole_episodes=True, entry="run_pairs")


def test_parsers_accept_the_flags():
    t = train.build_arg_parser()
    assert t.parse_args(["--config", "x.yaml"]).whole_episode_eval is None
    assert t.parse_args(["--config", "x.yaml", "--whole-episode-eval"]).whole_episode_eval is True
    assert t.parse_args(["--config", "x.yaml", "--per-step-eval"]).whole_episode_eval is False
    d = train_dock.build_arg_parser()
    required = [x for act in d._actions if act.required for x in (act.option_strings[0], "x")]
    assert d.parse_args(required).whole_episode_eval is None
    assert d.parse_args([*required, "--whole-episode-eval"]).whole_episode_eval is True
    assert d.parse_args([*required, "--per-step-eval"]).whole_episode_eval is False
    for parser, base in ((t, ["--config", "x.yaml"]), (d, required)):
        with pytest.raises(SystemExit):
            parser.parse_args([*base, "--whole-episode-eval", "--per-step-eval"])
