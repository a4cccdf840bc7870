"""The one training loop (ppo.run_training), the trainers' status lines, the shared CLI layer (trainer_cli) and the one-handle populations'
constructor, without a GPU: the loop on a stub trainer, every status line against a literal, the three parsers against the record of the
parsers as they stood before the shared layer (tests/golden/trainer_cli_flags.json), and the order of the constructor's first refusals."""
from __future__ import annotations

import argparse
import importlib.util
import json
import types

import pytest
import torch

from conftest import GOLDEN
from rl_brain_trainer_amd import ppo as kppo
from rl_brain_trainer_amd import population as kpop
from rl_brain_trainer_amd import train_dock, train_route, trainer_cli
from rl_brain_trainer_amd.ppo import PPOConfig


# ---------------------------------------------------------------------------------------------------------------- the driver
class _StubTrainer:
    """what run_training touches of a trainer; every iteration takes ``per_iter`` steps; make_loggers is PPO's own (real TrainLoggers)"""

    def __init__(self, *, per_iter: int = 100, K: int = 1, monitor: bool = False, rank: int = 0) -> None:
        self.num_timesteps, self.per_iter, self.K = 0, per_iter, K
        self.monitor = object() if monitor else None
        self.dist = types.SimpleNamespace(rank=rank)
        self.device = "stub-device"
        self.replica_names = [f"seed_{7 + k}" for k in range(K)]
        self.calls: list = []
        self.loggers: list = []

    def collect_rollouts(self) -> None:
        self.calls.append("collect")
        self.num_timesteps += self.per_iter

    def train(self) -> None:
        self.calls.append("train")

    def make_loggers(self, csv_paths):
        self.loggers = kppo.PPO.make_loggers(self, csv_paths)
        return self.loggers

    def monitor_rows(self):
        return [{"rollout/episodes": 10 * len(self.calls) + k} for k in range(self.K)]


@pytest.fixture
def synced(monkeypatch):
    seen = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: seen.append(device))
    return seen


def _status(trainer, it, steps, elapsed) -> str:
    assert elapsed >= 0.0
    return f"<status it={it} steps={steps} clock={trainer.num_timesteps}>"


def test_driver_order_termination_and_return(synced):
    t = _StubTrainer()
    t.num_timesteps = 5000                      # a start clock that is not zero (a resumed run)
    hooks = {"after_rollout": lambda tr: tr.calls.append("after_rollout"),
             "after_update": lambda tr, steps: tr.calls.append(("after_update", steps))}
    wall, steps = kppo.run_training(t, 250, **hooks)
    # 100 steps per iteration: the third iteration is the first that reaches 250
    assert t.calls == ["collect", "after_rollout", "train", ("after_update", 100), "collect", "after_rollout", "train", ("after_update", 200),
                       "collect", "after_rollout", "train", ("after_update", 300)]
    assert steps == 300 and t.num_timesteps == 5300 and wall >= 0.0
    assert synced == ["stub-device"]            # one synchronise of the trainer's device, before the wall time is taken
    t2 = _StubTrainer()
    assert kppo.run_training(t2, 300)[1] == 300 and t2.calls.count("collect") == 3     # reaching the total exactly ends the loop
    assert kppo.run_training(_StubTrainer(), 0)[1] == 0


@pytest.mark.parametrize("log_every, logged", [(0, []), (1, [1, 2, 3, 4]), (2, [2, 4]), (3, [3])])
def test_driver_log_cadence(synced, capsys, log_every, logged):
    kppo.run_training(_StubTrainer(), 400, log_every=log_every, status=_status)
    assert capsys.readouterr().out.splitlines() == [f"<status it={it} steps={100 * it} clock={100 * it}>" for it in logged]


def test_driver_status_on_rank_zero_only_and_never_with_a_monitor(synced, capsys):
    kppo.run_training(_StubTrainer(rank=1), 200, log_every=1, status=_status)
    assert capsys.readouterr().out == ""
    kppo.run_training(_StubTrainer(), 200, log_every=1)             # no status function: nothing to print
    assert capsys.readouterr().out == ""
    t = _StubTrainer(monitor=True)
    kppo.run_training(t, 200, log_every=1, status=_status)
    out = capsys.readouterr().out
    assert "<status" not in out and out.count("episodes") == 2 and "replica" not in out     # one table per iteration, no tag: no replica line


def test_driver_monitor_records_of_a_population(synced, capsys, tmp_path):
    t = _StubTrainer(K=2, monitor=True)
    t.num_timesteps = 700                       # the clock moved after the trainer was made (an init checkpoint): the loggers start from here
    paths = [tmp_path / "a" / "progress.csv", tmp_path / "b" / "progress.csv"]
    kppo.run_training(t, 400, log_every=2, status=_status, csv_paths=paths, tag="ppo-population")
    assert [lg._start_steps for lg in t.loggers] == [700, 700] and [lg.csv_path for lg in t.loggers] == paths
    lines = capsys.readouterr().out.splitlines()
    heads = [i for i, l in enumerate(lines) if l.startswith("[ppo-population]")]
    assert [lines[i] for i in heads] == ["[ppo-population] it=2 replica seed_7", "[ppo-population] it=2 replica seed_8",
                                         "[ppo-population] it=4 replica seed_7", "[ppo-population] it=4 replica seed_8"]
    # two records per logged iteration, each a table straight after its replica line, with this run's steps in it
    for n, i in enumerate(heads):
        end = heads[n + 1] if n + 1 < len(heads) else len(lines)
        table = lines[i + 1:end]
        assert table[0].startswith("---") and table[-1].startswith("---") and sum("episodes" in l for l in table) == 1, table
        assert any("total_timesteps" in l and str(700 + (200 if n < 2 else 400)) in l for l in table)
    for p in paths:
        rows = p.read_text().splitlines()
        assert len(rows) == 3 and [r.split(",")[5] for r in rows[1:]] == ["2", "4"]      # time/iterations


def test_ppo_learn_runs_the_driver(synced, capsys):
    p = object.__new__(kppo.PPO)
    seen = {}

    def fake(trainer, total, **kw):
        seen.update(trainer=trainer, total=total, **kw)
        return 0.0, total

    p.cfg = PPOConfig(total_timesteps=1234)
    orig, kppo.run_training = kppo.run_training, fake
    try:
        assert p.learn(log_every=3) is p
    finally:
        kppo.run_training = orig
    assert seen == {"trainer": p, "total": 1234, "log_every": 3, "status": kppo.status_line}
    assert not hasattr(kpop, "learn_population")


# ---------------------------------------------------------------------------------------------------------------- the status lines
STATS = {"policy_loss": -0.0125, "value_loss": 0.5, "n_updates": 8}


def _tracker(stage: int):
    return types.SimpleNamespace(read=lambda: types.SimpleNamespace(stage_index=stage))


def test_status_line_of_ppo_learn_and_train():
    p = types.SimpleNamespace(K=1, num_timesteps=10240, curricula=[_tracker(4)], rew_buf=torch.tensor([0.5, 0.25]), _stats_rows=lambda: [STATS])
    assert kppo.status_line(p, 3, 6144, 2.0) == "[ppo] it=3 steps=10240 fps=3,072 stage=4 rew=0.3750 {'policy_loss': -0.0125, 'value_loss': 0.5, 'n_updates': 8}"
    p.curricula = [None]
    assert kppo.status_line(p, 3, 6144, 2.0).split(" rew=")[0] == "[ppo] it=3 steps=10240 fps=3,072 stage=-1"
    p.K, p.curricula, p._stats_rows = 2, [_tracker(4), None], lambda: [STATS, {}]
    assert kppo.status_line(p, 1, 2_000_000, 0.5) == ("[ppo] it=1 steps=10240 fps=4,000,000 stage=[4, -1] rew=0.3750 "
                                                      "[{'policy_loss': -0.0125, 'value_loss': 0.5, 'n_updates': 8}, {}]")


def test_status_line_of_train_dock():
    p = types.SimpleNamespace(num_timesteps=4096, curriculum=types.SimpleNamespace(current_stage_index=1), rew_buf=torch.tensor([-1.0, 0.5]), last_stats=STATS)
    assert train_dock.status_line(p, 2, 4096, 4.0) == "[ppo-dock] it=2 steps=4096 fps=1,024 stage=1 rew=-0.2500 {'policy_loss': -0.0125, 'value_loss': 0.5, 'n_updates': 8}"
    p.curriculum = None
    assert " stage=-1 " in train_dock.status_line(p, 2, 4096, 4.0)


def test_status_line_of_train_route():
    cur = types.SimpleNamespace(summary=lambda: {"prefix_end_index": 20, "recent_success_rate": 0.4375})
    p = types.SimpleNamespace(num_timesteps=36864, curriculum=cur, rew_buf=torch.tensor([0.125]))
    assert train_route.status_line(p, 5, 4096, 0.25) == "[route] it=5 steps=36864 fps=16,384 prefix=20 succ=0.438 rew=0.1250 anchor=0.00000"
    anchor = types.SimpleNamespace(last_loss=0.0123456)
    assert train_route.status_line(p, 5, 4096, 0.25, anchor=anchor).endswith(" rew=0.1250 anchor=0.01235")


def test_status_lines_of_the_populations():
    pop = types.SimpleNamespace(K=3, num_timesteps=2048, curricula=[_tracker(2), None, _tracker(0)])
    assert kpop.population_status(pop, 2, 2048, 3.0, tag="ppo-dock-population") == \
        "[ppo-dock-population] it=2 steps/replica=2048 aggregate fps=2,048 stages=[2, -1, 0]"
    assert kpop.population_status(pop, 2, 2048, 3.0).startswith("[population] it=2 ")
    cur = types.SimpleNamespace(summary=lambda k: {"prefix_end_index": 10 * (k + 1)})
    rp = types.SimpleNamespace(K=2, num_timesteps=5120, pop_curriculum=cur, teacher_anchor=None)
    assert train_route.population_status_line(rp, 4, 4096, 2.0) == "[route-population] it=4 steps/replica=5120 aggregate fps=4,096 prefixes=[10, 20]"
    rp.teacher_anchor = types.SimpleNamespace(last_loss=[0.1234567, 0.5])
    assert train_route.population_status_line(rp, 4, 4096, 2.0) == ("[route-population] it=4 steps/replica=5120 aggregate fps=4,096 prefixes=[10, 20] "
                                                                   "anchor=[0.12346, 0.5]")


# ---------------------------------------------------------------------------------------------------------------- the parsers
def test_parsers_hold_every_flag_as_before_the_shared_layer():
    spec = importlib.util.spec_from_file_location("make_golden_trainer_cli_flags", GOLDEN / "make_golden_trainer_cli_flags.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.loads((GOLDEN / "trainer_cli_flags.json").read_text())
    got = json.loads(json.dumps(gen.records()))
    assert sorted(got) == sorted(want) == ["train", "train_dock", "train_route"]
    for module in want:
        assert sorted(got[module]) == sorted(want[module]), module
        for flag in want[module]:
            assert got[module][flag] == want[module][flag], (module, flag)
    assert sum(len(v) for v in want.values()) > 60 and want["train"]["--train-tile"]["exclusive_with"] == ["--per-step-rollout", "--train-tile", "--whole-rollout"]


# ---------------------------------------------------------------------------------------------------------------- the CLI layer
def test_apply_switches_exports_where_the_parser_has_the_flag(monkeypatch):
    for var in ("KP1_TRAIN_TILE", "KP1_ROLLOUT_RUN", "KP1_FUSED_ROUTE_ROLLOUT"):
        monkeypatch.delenv(var, raising=False)
    import os

    trainer_cli.apply_switches(argparse.Namespace(sweep=None, seeds=None))                       # a parser with none of the three flags
    trainer_cli.apply_switches(argparse.Namespace(sweep=None, seeds=None, train_tile=False, whole_rollout=None, one_launch_rollout=False))
    assert not {"KP1_TRAIN_TILE", "KP1_ROLLOUT_RUN", "KP1_FUSED_ROUTE_ROLLOUT"} & set(os.environ)
    trainer_cli.apply_switches(argparse.Namespace(sweep=["gamma=0.9,0.99"], seeds="7", train_tile=True, whole_rollout=False, one_launch_rollout=True))
    assert (os.environ["KP1_TRAIN_TILE"], os.environ["KP1_ROLLOUT_RUN"], os.environ["KP1_FUSED_ROUTE_ROLLOUT"]) == ("1", "0", "1")
    trainer_cli.apply_switches(argparse.Namespace(sweep=None, seeds=None, whole_rollout=True))
    assert os.environ["KP1_ROLLOUT_RUN"] == "1"
    with pytest.raises(ValueError, match="--sweep needs --seeds"):
        trainer_cli.apply_switches(argparse.Namespace(sweep=["gamma=0.9"], seeds=None, train_tile=True))


@pytest.fixture
def process(monkeypatch):
    """torch.cuda.set_device and the process-group calls recorded instead of made"""
    import torch.distributed as dist

    seen: list = []
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: seen.append(("set_device", d)))
    monkeypatch.setattr(dist, "init_process_group", lambda **kw: seen.append(("init", kw["backend"], kw["device_id"].index)))
    monkeypatch.setattr(dist, "destroy_process_group", lambda: seen.append("destroy"))
    monkeypatch.setattr(dist, "barrier", lambda: seen.append("barrier"))
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR"):
        monkeypatch.delenv(var, raising=False)
    return seen


def _dp_trainer(seen, enabled: bool):
    return types.SimpleNamespace(dist=types.SimpleNamespace(enabled=enabled, close=lambda: seen.append("close")))


def test_process_context_single_process(process, monkeypatch):
    with trainer_cli.process_context(argparse.Namespace()) as proc:               # no --device flag, no LOCAL_RANK
        assert (proc.world, proc.rank, proc.device, proc.own_group) == (1, 0, 0, False)
        proc.trainer = _dp_trainer(process, False)
    with trainer_cli.process_context(argparse.Namespace(device=3)) as proc:
        assert proc.device == 3
    monkeypatch.setenv("LOCAL_RANK", "5")
    with trainer_cli.process_context(argparse.Namespace(device=3)) as proc:       # LOCAL_RANK beats --device
        assert proc.device == 5
    assert process == [("set_device", 0), ("set_device", 3), ("set_device", 5)]   # no group, no barrier, nothing closed


def test_process_context_owns_the_group_it_makes(process, monkeypatch):
    import os

    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("LOCAL_RANK", "1")
    with trainer_cli.process_context(argparse.Namespace()) as proc:
        assert (proc.world, proc.rank, proc.device, proc.own_group) == (2, 1, 1, True) and os.environ["MASTER_ADDR"] == "127.0.0.1"
        proc.trainer = _dp_trainer(process, True)
    assert process == [("set_device", 1), ("init", "nccl", 1), "barrier", "close", "destroy"]
    process.clear()
    with pytest.raises(ValueError, match="one GPU"):                              # a refusal inside: no barrier to hang on, the group still goes
        with trainer_cli.process_context(argparse.Namespace()) as proc:
            trainer_cli.refuse_population_under_dp(proc.world)
    assert process == [("set_device", 1), ("init", "nccl", 1), "destroy"]
    trainer_cli.refuse_population_under_dp(1)


def test_process_context_uses_the_callers_group(process, monkeypatch):
    import torch.distributed as dist

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 4)
    monkeypatch.setattr(dist, "get_rank", lambda: 2)
    with trainer_cli.process_context(argparse.Namespace(device=0)) as proc:
        assert (proc.world, proc.rank, proc.own_group) == (4, 2, False)
        proc.trainer = _dp_trainer(process, True)
    assert process == [("set_device", 0), "barrier", "close"]                     # used, not initialised again, not destroyed


def test_replica_extra_and_write_json(tmp_path):
    assert trainer_cli.replica_extra(7, "seed_7", None) == {"seed": 7}
    o = {"learning_rate": 1e-4}
    extra = trainer_cli.replica_extra(7, "seed_7_learning_rate_0.0001", o)
    assert extra == {"seed": 7, "replica": "seed_7_learning_rate_0.0001", "overrides": o} and extra["overrides"] is not o
    trainer_cli.write_json(tmp_path / "a" / "b.json", {"x": [1, 2]})
    assert (tmp_path / "a" / "b.json").read_text() == json.dumps({"x": [1, 2]}, indent=2)
    trainer_cli.write_json(tmp_path / "c.json", {"p": tmp_path}, default=str)
    assert json.loads((tmp_path / "c.json").read_text()) == {"p": str(tmp_path)}
    with pytest.raises(TypeError):
        trainer_cli.write_json(tmp_path / "d.json", {"p": tmp_path})


# ---------------------------------------------------------------------------------------------------------------- the one-handle constructor
def _bare(cls, **attrs):
    obj = cls.__new__(cls)
    obj.__dict__.update(attrs, _handle=None)
    return obj


def _wrong_envs():
    from rl_brain_trainer_amd.vec_env import ArmKinematicPopulationVecEnv, ArmKinematicVecEnv

    approach_mode = types.SimpleNamespace(mode_name="approach")
    return {"ApproachPopulationPPO": _bare(ArmKinematicVecEnv, seeds=[1, 2]), "RoutePopulationPPO": types.SimpleNamespace(seeds=[1, 2]),
            "DockPopulationPPO": _bare(ArmKinematicPopulationVecEnv, seeds=[1, 2], config=approach_mode)}


@pytest.mark.parametrize("cls_name, words", [("ApproachPopulationPPO", "drives an ArmKinematicPopulationVecEnv"),
                                             ("RoutePopulationPPO", "drives a RoutePopulationVecEnv"),
                                             ("DockPopulationPPO", "drives a dock-mode ArmKinematicPopulationVecEnv")])
def test_one_handle_constructor_refuses_the_env_type_before_the_seeds(cls_name, words, monkeypatch):
    """an env that is of the wrong type AND made for other seeds: the type is refused first; the arguments' own refusals come before both"""
    from rl_brain_trainer_amd import native

    def touched(*_a, **_k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(native, "load", touched)
    cls = getattr(kpop, cls_name)
    assert "__init__" not in cls.__dict__ and cls.__init__ is kpop.OneHandlePopulationPPO.__init__
    env = _wrong_envs()[cls_name]
    with pytest.raises(TypeError, match=f"{cls_name} {words} \\(one handle for all replicas\\)"):
        cls([7, 8], PPOConfig(hidden=64), env)
    with pytest.raises(ValueError, match="hidden=256"):
        cls([7, 8], PPOConfig(hidden=256), env)
    right = _bare(cls.env_class, seeds=[1, 2], config=types.SimpleNamespace(mode_name="dock"))
    with pytest.raises(ValueError, match=f"the {cls.env_class.__name__} was made for seeds \\[1, 2\\], not \\[7, 8\\]"):
        cls([7, 8], PPOConfig(hidden=64), right, curriculum=object())      # (a wrong tracker too: the seeds are refused before it)
