"""The host side of the one-launch route chain evaluator without a GPU: the two symbols are declared, exported and bound, the header's span cap
equals the Python constants, the predicate that says which handles the kernels cover (route_curriculum.chain_fused_covered) on plain values,
the library's NULL refusals, how evaluate_sequential_route_batch chooses its form (on fakes, before any device work) and how the whole-chain
form's ``lock_steps`` rounds."""
from __future__ import annotations

import ctypes as C
import json
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import route_config as rcfg
from rl_brain_trainer_amd import route_curriculum as rc

F32, F64 = torch.float32, torch.float64
SYMBOLS = {"kp1_mlp_forward_route_chain_step": 11, "kp1_route_chain_run": 9}


def test_symbols_declared_exported_and_bound():
    declared = native.declared_symbols()
    L = native.load()
    for name, n_args in SYMBOLS.items():
        assert name in declared
        fn = getattr(L, name)                     # exported by libkp1.so
        assert fn.argtypes is not None and len(fn.argtypes) == n_args, name      # bound by native.load()


def test_span_cap_matches_the_header():
    header = (kcfg.repo_root() / "include" / "kp1_route.h").read_text()
    m = re.search(r"#define\s+KP1_ROUTE_CHAIN_RUN_MAX_STEPS\s+(\d+)", header)
    assert m and int(m.group(1)) == native.ROUTE_CHAIN_RUN_MAX_STEPS == rc.CHAIN_RUN_MAX_STEPS == 1024
    m = re.search(r"#define\s+KP1_ROUTE_FUSED_MAX_WAYPOINTS\s+(\d+)", header)
    assert m and int(m.group(1)) == rc.CHAIN_FUSED_MAX_WAYPOINTS


def _covered(dtype=F32, hidden=64, obs_dim=80, pitch=128, components_on=False, n_waypoints=484):
    return rc.chain_fused_covered(dtype, hidden, obs_dim, pitch, components_on, n_waypoints)


def test_predicate_on_plain_values():
    for hidden in (64, 128):
        for obs_dim, pitch in ((56, 56), (56, 64), (80, 80), (80, 128)):
            assert _covered(hidden=hidden, obs_dim=obs_dim, pitch=pitch)
    assert not _covered(dtype=F64)
    assert not _covered(hidden=256)
    assert not _covered(hidden=32)
    assert not _covered(obs_dim=64, pitch=64)      # the observation width, not the pitch
    assert not _covered(obs_dim=56, pitch=128)
    assert not _covered(obs_dim=80, pitch=96)
    assert not _covered(components_on=True)
    assert _covered(n_waypoints=rc.CHAIN_FUSED_MAX_WAYPOINTS)
    assert not _covered(n_waypoints=rc.CHAIN_FUSED_MAX_WAYPOINTS + 1)


def test_null_refusals_without_a_device():
    L = native.load()
    buf = np.zeros(64, dtype=np.float32)
    p = C.c_void_p(buf.ctypes.data)
    assert L.kp1_mlp_forward_route_chain_step(None, None, None, p, 80, None, p, p, p, None, None) != native.KP1_OK
    assert b"NULL argument to kp1_mlp_forward_route_chain_step" in L.kp1_last_error()
    assert L.kp1_route_chain_run(None, None, None, p, 80, p, p, 4, None) != native.KP1_OK
    assert b"NULL argument to kp1_route_chain_run" in L.kp1_last_error()
    assert not buf.any()


def test_form_selection_on_plain_values():
    assert rc.CHAIN_FORMS == ("launch_sequence", "one_launch_step", "whole_chain")
    assert rc.CHAIN_FORM_DEFAULT in rc.CHAIN_FORMS
    for covered in (True, False):
        assert rc.chain_form_selected("launch_sequence", covered) == "launch_sequence"
        assert rc.chain_form_selected(None, covered) == (rc.CHAIN_FORM_DEFAULT if covered else "launch_sequence")
    for form in ("one_launch_step", "whole_chain"):
        assert rc.chain_form_selected(form, True) == form
        with pytest.raises(ValueError, match="one-launch chain kernels"):
            rc.chain_form_selected(form, False)
    with pytest.raises(ValueError, match="form must be"):
        rc.chain_form_selected("whole-chain", True)


def test_default_falls_back_silently_when_a_one_launch_form_is_the_default(monkeypatch):
    monkeypatch.setattr(rc, "CHAIN_FORM_DEFAULT", "whole_chain")
    assert rc.chain_form_selected(None, True) == "whole_chain"
    assert rc.chain_form_selected(None, False) == "launch_sequence"


class _FakeMlp:
    """what evaluate_sequential_route_batch reads of a policy handle before it touches the device"""

    def __init__(self, hidden: int, obs_dim: int = 80) -> None:
        self.hidden, self.obs_dim, self.replicas, self.max_batch = hidden, obs_dim, 1, 8
        self.obs_pad = 64 if obs_dim <= 64 else 128


def _batch(**kw):
    cfg = json.loads((GOLDEN / "configs" / "route_curriculum_prefix120_routeobs_sequence2.json").read_text())
    route_q = rcfg.load_route_q(GOLDEN / "synthetic_route.json")
    return rc.evaluate_sequential_route_batch(cfg=cfg, route_q=route_q, start_index=1, end_indices=[3], **kw)


def test_a_named_form_that_is_not_covered_raises_before_any_device_work():
    for form in ("one_launch_step", "whole_chain"):
        with pytest.raises(ValueError, match="one-launch chain kernels"):
            _batch(mlp=_FakeMlp(256), form=form)
    with pytest.raises(ValueError, match="form must be"):
        _batch(mlp=_FakeMlp(64), form="persistent")
    for span in (0, rc.CHAIN_RUN_MAX_STEPS + 1):
        with pytest.raises(ValueError, match="steps_per_launch"):
            _batch(mlp=_FakeMlp(64), form="whole_chain", steps_per_launch=span)


def test_lock_steps_rounding():
    """the whole-chain form issues whole spans until the counter reads zero, never past the bound; at 32 it is the launch-sequence count"""
    def launch_sequence(needed, bound):
        steps = 0
        while steps < bound:
            steps += 1
            if steps % rc._ALIVE_CHECK_EVERY == 0 and steps >= needed:
                break
        return steps

    for needed, bound in ((1, 288), (32, 288), (33, 288), (192, 288), (280, 288), (288, 288), (10, 24), (24, 24), (100, 1000)):
        assert rc.chain_lock_steps(needed, 32, bound) == launch_sequence(needed, bound), (needed, bound)
    assert rc.chain_lock_steps(33, 256, 1000) == 256
    assert rc.chain_lock_steps(257, 256, 1000) == 512
    assert rc.chain_lock_steps(257, 256, 400) == 400
    assert rc.chain_lock_steps(5, 1024, 288) == 288
    assert rc.chain_lock_steps(7, 7, 288) == 7


def test_cli_flags():
    from rl_brain_trainer_amd import collect_route_teacher, train_route

    base = ["--config", "x.yaml", "--run-id", "r", "--seeds", "1,2"]
    assert train_route.build_arg_parser().parse_args(base).chain_eval_form is None
    for form in ("launch-sequence", "one-launch-step", "whole-chain"):
        assert train_route.build_arg_parser().parse_args(base + ["--chain-eval-form", form]).chain_eval_form == form
        assert form.replace("-", "_") in rc.CHAIN_FORMS
    rec = ["--checkpoint", "m.zip", "--config", "x.yaml", "--route-path", "r.json", "--artifact-root", "out"]
    assert not collect_route_teacher.build_arg_parser().parse_args(rec).one_launch
    assert collect_route_teacher.build_arg_parser().parse_args(rec + ["--one-launch"]).one_launch
