"""The host side of the one-launch evaluation step for 2x256 policies, without a GPU: which handles the predicate covers, how a policy
callable resolves to its handle, the ``one_launch`` keyword of the evaluators and the CLI flag."""
from __future__ import annotations

import inspect
import types

import pytest

from rl_brain_trainer_amd import evaluate as ev
from rl_brain_trainer_amd import train, train_dock
from rl_brain_trainer_amd import workspace_coverage as wc


def _fake_mlp(hidden=256, obs_dim=56, replicas=1, fused=True):
    return types.SimpleNamespace(hidden=hidden, obs_dim=obs_dim, replicas=replicas, fused=fused)


def test_is_fused_width_covers_the_tile_path_of_hidden_256():
    assert ev._is_fused_width(_fake_mlp())
    assert not ev._is_fused_width(_fake_mlp(fused=False))          # switched to the layer-wise kernels: kp1_eval_step refuses it
    assert not ev._is_fused_width(_fake_mlp(obs_dim=80))
    assert not ev._is_fused_width(_fake_mlp(replicas=3))
    assert not ev._is_fused_width(None)
    # the layer-wise widths as before, population handles included
    for hidden in (64, 128):
        assert ev._is_fused_width(_fake_mlp(hidden=hidden)) and ev._is_fused_width(_fake_mlp(hidden=hidden, replicas=3))
        assert not ev._is_fused_width(_fake_mlp(hidden=hidden, obs_dim=80))
    assert not ev._is_fused_width(_fake_mlp(hidden=32))


class _Policy:
    def __init__(self, mlp):
        self._mlp = mlp

    def predict(self, obs, deterministic=True):
        return obs

    def predict_unclipped(self, obs):
        return obs

    __call__ = predict


def test_policy_mlp_resolves_instances_and_bound_predict_only():
    mlp = _fake_mlp()
    pol = _Policy(mlp)
    assert ev.policy_mlp(pol) is mlp
    assert ev.policy_mlp(pol.predict) is mlp
    assert ev.policy_mlp(pol.predict_unclipped) is None          # another method of the same object is not the clipped deterministic policy
    assert ev.policy_mlp(lambda obs: pol.predict(obs)) is None

    def plain(obs):
        return obs

    assert ev.policy_mlp(plain) is None
    assert ev.policy_mlp(types.SimpleNamespace()) is None


def test_one_launch_switch_on_fakes():
    """False never resolves a handle; True raises for what is not covered; a population handle behind a policy is not a K = 1 policy"""
    pol = _Policy(_fake_mlp())
    assert ev._one_launch_mlp(pol.predict, object(), False, "Approach") is None
    with pytest.raises(ValueError, match="one_launch=True: the Approach phase"):
        ev._one_launch_mlp(lambda o: o, object(), True, "Approach")
    with pytest.raises(ValueError, match="one_launch=True"):
        ev._one_launch_mlp(pol.predict, object(), True, "Finisher")          # covered handle, but not an ArmKinematicVecEnv
    assert ev._one_launch_mlp(pol.predict, object(), None, "Approach") is None
    assert ev._one_launch_mlp(_Policy(_fake_mlp(hidden=64, replicas=3)).predict, object(), None, "Approach") is None


@pytest.mark.parametrize("fn", [ev.evaluate_workspace_expansion, wc.run_pairs, wc.evaluate_full_workspace_coverage, wc._run_pairs_columns,
                                train_dock.evaluate_dock])
def test_one_launch_is_a_keyword_defaulting_to_none(fn):
    p = inspect.signature(fn).parameters["one_launch"]
    assert p.default is None and p.kind in (inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD)


def test_parsers_accept_the_evaluation_flags():
    a = train.build_arg_parser().parse_args(["--config", "x.yaml", "--multi-launch-eval"])
    assert a.multi_launch_eval is True
    assert train.build_arg_parser().parse_args(["--config", "x.yaml"]).multi_launch_eval is False
    d = train_dock.build_arg_parser()
    required = [x for act in d._actions if act.required for x in (act.option_strings[0], "x")]
    # train_dock.py keeps the launch sequence as its default (its evaluation has not been timed): the flag there switches the one-launch step on
    assert d.parse_args([*required, "--one-launch-eval"]).one_launch_eval is True
    assert d.parse_args(required).one_launch_eval is False


def test_population_evaluator_still_refuses_hidden_256():
    pop = types.SimpleNamespace(K=3, obs_dim=56, obs_w=64, cfg=types.SimpleNamespace(hidden=256), _mlp=None)
    with pytest.raises(ValueError, match="hidden=256"):
        ev.evaluate_workspace_expansion_population(population=pop, finisher_policy=None, approach_cfg=None, finisher_cfg=None, artifact_roots=None)
