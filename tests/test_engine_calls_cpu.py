"""The PPO engine's Python half without a device: ``PPO``, the K-handle ``PopulationPPO`` and ``ApproachPopulationPPO``
stood on CPU tensors, and the exact ordered sequence of calls that a rollout step, a rollout, the rollout tail and ``train()`` make -- to
the library, to the MLP handle, to the env handles, the trackers, the monitor and the collectives -- with their arguments; and the names of
the aten operations that ``_post_rollout()`` and ``_epoch_body()`` issue, which is the launch sequence as far as Python decides it.

How the trainers stand here.  The real constructors run (``_setup`` / ``_init_population``), so every buffer has its real shape.
``native.load`` gives a recording library (every ``kp1_*`` call returns 0), ``mlp.MlpKernels`` and ``monitor.EpisodeMonitor`` are recording
objects, ``torch.cuda.current_stream`` is a stub with a known address, the env handles and trackers are instances of the real classes made
without their constructors whose ``step_into``, ``reset``, ``observe``, ``set_obs_stride`` and ``attach`` record, and the ``Dist`` is a
fake whose collectives record when it is enabled (the real one's are no-ops otherwise).

How calls are compared.  A scalar by its value; ``None`` as ``None``; a pointer as (the trainer buffer it points into, its element offset),
found by looking the address up in a table of the trainer's tensors; a tensor handed over as an object as (buffer, offset, shape); a
temporary as ``tmp<shape of its allocation>:<dtype>`` in place of the buffer name (every tensor made while the recorder is active is kept
alive, so no address is used twice).  The expected lists are built below from the geometry, one builder per step of an iteration."""
from __future__ import annotations

import ctypes as C
import types

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_flatten

from rl_brain_trainer_amd import curriculum as kcur
from rl_brain_trainer_amd import mlp as kmlp
from rl_brain_trainer_amd import monitor as kmon
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import population as kpop
from rl_brain_trainer_amd import ppo as kppo
from rl_brain_trainer_amd import vec_env as ve

CPU = torch.device("cpu")
STREAM = 0x5150
T, N, W, A = 4, 3, 64, 7                 # n_steps, envs per replica, observation pitch, action width
MAX_EPISODE_STEPS = 2                    # -> the bootstrap's index list holds N * (T // 2 + 1) = 9 rows per replica
CAP = 9
ENV_VARS = ("KP1_FUSED_ROLLOUT", "KP1_ROLLOUT_RUN", "KP1_FUSED_ROUTE_ROLLOUT", "KP1_TRAIN_TILE", "KP1_BF16X3_WGRAD", "KP1_DONE_EXCHANGE_STEPS",
            "KP1_DP_EPOCH")
CONFIG = types.SimpleNamespace(c=types.SimpleNamespace(termination=types.SimpleNamespace(max_episode_steps=MAX_EPISODE_STEPS)), mode_name="approach")
F32, F64, I64 = "torch.float32", "torch.float64", "torch.int64"


class _Rec(TorchDispatchMode):
    """the recorder: the calls in order, the aten operations in order, and every allocation made meanwhile"""

    def __init__(self) -> None:
        super().__init__()
        self.calls: list[tuple] = []
        self.ops: list[str] = []
        self.quiet = False               # a fake writing what a kernel would write: no operation of the code under test
        self.pool: dict[int, torch.Tensor] = {}
        self.objects: dict[int, str] = {}
        self.trainer = None

    def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if not self.quiet:
            self.ops.append(str(func).removeprefix("aten."))
        for t in tree_flatten(out)[0]:
            if isinstance(t, torch.Tensor) and t.untyped_storage().nbytes():
                self.pool.setdefault(t.untyped_storage().data_ptr(), t)
        return out

    def name(self, obj, name: str):
        self.objects[id(obj)] = name
        return obj

    def add(self, name: str, *args, **kwargs) -> None:
        self.calls.append((name, args, kwargs))

    def method(self, owner: str, name: str, ret=None):
        def call(*args, **kwargs):
            self.add(f"{owner}.{name}", *args, **kwargs)
            return ret() if ret is not None else None
        return call

    # ---- resolution
    def _owner(self, addr: int) -> tuple:
        for key, t in vars(self.trainer).items():
            if isinstance(t, torch.Tensor) and t.data_ptr() <= addr < t.data_ptr() + t.numel() * t.element_size():
                return key, (addr - t.data_ptr()) // t.element_size()
        for base, t in self.pool.items():
            if base <= addr < base + t.untyped_storage().nbytes():
                return f"tmp{tuple(t.shape)}:{t.dtype}", (addr - base) // t.element_size()
        raise AssertionError(f"address {addr:#x} is in no tensor the recorder knows")

    def _item(self, a):
        if a is None or isinstance(a, (bool, int, float, str)):
            return a
        if isinstance(a, torch.Tensor):
            return (*self._owner(a.data_ptr()), tuple(a.shape))
        if isinstance(a, C.c_void_p):
            return None if not a.value else "stream" if a.value == STREAM else self._owner(a.value)
        if isinstance(a, (list, tuple)):
            return [self._item(x) for x in a]
        if isinstance(a, dict):
            return {k: self._item(v) for k, v in a.items()}
        if id(a) in self.objects:
            return self.objects[id(a)]
        raise AssertionError(f"no rule for argument {a!r}")

    def take(self) -> list[tuple]:
        """the calls since the last take(), resolved: (name, *positional, {keywords}) -- the dict only where there are keywords"""
        out = [(name, *[self._item(a) for a in args], *([{k: self._item(v) for k, v in kwargs.items()}] if kwargs else []))
               for name, args, kwargs in self.calls]
        self.calls = []
        return out

    def take_ops(self) -> list[str]:
        out, self.ops = self.ops, []
        return out


class _Lib:
    def __init__(self, rec: _Rec) -> None:
        self.rec = rec

    def __getattr__(self, name: str):
        if not name.startswith("kp1_"):
            raise AttributeError(name)

        def call(*args):
            self.rec.add(name, *args)
            return 0
        return call


class _Mlp:
    """the recording MLP handle.  ``forward`` with a ``value`` output writes VALUE there, as the critic would write its values"""
    HPARAM_FIELDS = kmlp.MlpKernels.HPARAM_FIELDS
    VALUE = 2.0
    rec: _Rec = None
    max_batch_cap = None                 # a test's smaller max_batch, so that PPO's bootstrap forward runs in chunks

    def __init__(self, hidden, device, max_batch=8192, obs_dim=56, replicas=1) -> None:
        self.rec.add("mlp.create", hidden, max_batch, obs_dim, replicas)
        self.max_batch = max_batch if self.max_batch_cap is None else self.max_batch_cap
        self.fused, self.train_tile, self.replicas = True, False, replicas

    def forward(self, obs, **kw) -> None:
        self.rec.add("mlp.forward", obs, **kw)
        if kw.get("value") is not None:
            self.rec.quiet = True
            kw["value"].fill_(self.VALUE)
            self.rec.quiet = False

    def __getattr__(self, name: str):
        if name.startswith("_"):
            raise AttributeError(name)
        return self.rec.method("mlp", name)


class _Monitor:
    rec: _Rec = None

    def __init__(self, device, K, N_, window=100, max_steps=0) -> None:
        self.rec.add("monitor.create", K, N_, window, max_steps)

    def __getattr__(self, name: str):
        if name.startswith("_"):
            raise AttributeError(name)
        return self.rec.method("monitor", name)


class _Dist:
    """``ppo.Dist`` as the trainers use it; the collectives record when enabled and are the real one's no-ops otherwise"""
    backend, rccl, _segments, rank = "fake", None, None, 0

    def __init__(self, rec: _Rec, world: int = 1) -> None:
        self.rec, self.world_size, self.enabled = rec, world, world > 1

    def broadcast(self, t, src=0):
        return t

    def use_stream_collectives(self, device) -> bool:
        return False

    def all_reduce_sum(self, t):
        if self.enabled:
            self.rec.add("dist.all_reduce_sum", t)
        return t

    def all_gather_into(self, out, t):
        if self.enabled:
            self.rec.add("dist.all_gather_into", out, t)
        return out


@pytest.fixture
def rec(monkeypatch):
    r = _Rec()
    monkeypatch.setattr(native, "load", lambda: _Lib(r))
    monkeypatch.setattr(kmlp, "MlpKernels", type("Mlp", (_Mlp,), {"rec": r}))
    monkeypatch.setattr(kmon, "EpisodeMonitor", type("Monitor", (_Monitor,), {"rec": r}))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda _d=None: types.SimpleNamespace(cuda_stream=STREAM))
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: types.SimpleNamespace())
    monkeypatch.setattr(torch.cuda, "Event", lambda *a, **k: types.SimpleNamespace(record=lambda *_: None))
    for var in ENV_VARS:
        monkeypatch.delenv(var, raising=False)
    with r:
        yield r


# ------------------------------------------------------------------------------------------------------------------------ fakes of envs, trackers
def _env(rec: _Rec, cls: type, n: int, name: str = "env", **attrs):
    """an instance of the real handle class ``cls`` (the trainers ask ``type(env) is`` / ``isinstance``) without its constructor"""
    env = rec.name(object.__new__(cls), name)
    env.__dict__.update(device=CPU, n_envs=n, dtype=torch.float32, _mode_name="approach", config=CONFIG, launch_args_version=0, obs_stride=56, **attrs)

    def set_obs_stride(stride):
        rec.add(f"{name}.set_obs_stride", stride)
        env.obs_stride = stride

    env.__dict__.update(set_obs_stride=set_obs_stride, step_into=rec.method(name, "step_into"), close=lambda: None,
                        reset=rec.method(name, "reset", ret=lambda: torch.zeros((n, W))), use_current_stream=rec.method(name, "use_current_stream"))
    return env


def _tracker(rec: _Rec, cls: type = kcur.PointCurriculum, name: str = "tracker", **attrs):
    cur = rec.name(object.__new__(cls), name)
    cur.__dict__.update(_st=C.c_void_p(), attach=rec.method(name, "attach"), observe=rec.method(name, "observe"),
                        observe_chunk=rec.method(name, "observe_chunk"), **attrs)
    return cur


def _cfg(batch_size: int = 4, **kw) -> kppo.PPOConfig:
    return kppo.PPOConfig(n_steps=T, batch_size=batch_size, n_epochs=2, hidden=64, learning_rate=1e-3, ent_coef=0.01, gamma=0.9, seed=5, **kw)


def _ppo(rec: _Rec, *, tracker: bool = False, world: int = 1, monitor: bool = False, **cfg):
    env = _env(rec, ve.ArmKinematicVecEnv, N)
    p = kppo.PPO(env, _cfg(**cfg), curriculum=_tracker(rec) if tracker else None, dist=_Dist(rec, world), use_graphs=False, monitor=monitor)
    rec.trainer = p
    return p


def _k_handle(rec: _Rec, K: int, *, tracker: bool = False, monitor: bool = False, **cfg):
    seeds = list(range(11, 11 + K))
    p = kpop.PopulationPPO(seeds, _cfg(**cfg), lambda s: _env(rec, ve.ArmKinematicVecEnv, N, f"env{s - 11}"),
                           curriculum_factory=(lambda s: _tracker(rec, name=f"tracker{s - 11}")) if tracker else None, dist=_Dist(rec),
                           use_graphs=False, monitor=monitor)
    rec.trainer = p
    return p


OVERRIDES = {"gamma": 0.8, "learning_rate": 5e-4}


def _approach(rec: _Rec, K: int, *, tracker: bool = False, overrides: bool = False, monitor: bool = False, **cfg):
    seeds = list(range(11, 11 + K))
    env = _env(rec, ve.ArmKinematicPopulationVecEnv, K * N, seeds=seeds, K=K, n_per_replica=N, is_population=True)
    cur = _tracker(rec, kcur.PointCurriculumPopulation, K=K) if tracker else None
    p = kpop.ApproachPopulationPPO(seeds, _cfg(**cfg), env, curriculum=cur, dist=_Dist(rec), use_graphs=False, monitor=monitor,
                                   overrides=[{}] * (K - 1) + [dict(OVERRIDES)] if overrides else None)
    rec.trainer = p
    return p


# ------------------------------------------------------------------------------------------------------------------------ expected calls
def tmp(shape: tuple, dtype: str, off: int = 0, view: tuple | None = None) -> tuple:
    return (f"tmp{tuple(shape)}:{dtype}", off) if view is None else (f"tmp{tuple(shape)}:{dtype}", off, tuple(view))


def step_buffers(t: int, KN: int, lo: int = 0, n: int | None = None) -> dict[str, tuple]:
    """rows [lo, lo + n) of step t's slice of every rollout buffer, as tensors handed over"""
    n = KN if n is None else n
    return {"obs": ("obs_buf", (t * KN + lo) * W, (n, W)), "noise": ("noise_all", (t * KN + lo) * A, (n, A)), "value": ("val_buf", t * KN + lo, (n,)),
            "action": ("act_buf", (t * KN + lo) * A, (n, A)), "clipped": ("clip_act", lo * A, (n, A)), "log_prob": ("logp_buf", t * KN + lo, (n,)),
            "next_obs": ("obs_buf", ((t + 1) * KN + lo) * W, (n, W)), "reward": ("rew_buf", t * KN + lo, (n,)), "done": ("done_buf", t * KN + lo, (n,)),
            "terminal_obs": ("term_obs_buf", (t * KN + lo) * W, (n, W))}


def launch_sequence_step(t: int, K: int, *, envs: list[str], trackers: list[str]) -> list[tuple]:
    """forward, then step_into per env handle, then observe per tracker (one handle: the whole width; K handles: a replica's columns each)"""
    KN = K * N
    b = step_buffers(t, KN)
    out = [("mlp.forward", b["obs"], {k: b[k] for k in ("noise", "value", "action", "clipped", "log_prob")})]
    n = KN // len(envs)
    for j, env in enumerate(envs):
        s = step_buffers(t, KN, j * n, n)
        out.append((f"{env}.step_into", s["clipped"], s["next_obs"], s["reward"], s["done"], s["terminal_obs"], True))
    for j, cur in enumerate(trackers):
        out.append((f"{cur}.observe", step_buffers(t, KN, j * (KN // len(trackers)), KN // len(trackers))["done"], N))
    return out


def fused_step(t: int, K: int, *, tracker: bool) -> list[tuple]:
    b = step_buffers(t, K * N)
    out = [("mlp.forward_env_step", "env", b["obs"], {k: b[k] for k in ("noise", "value", "action", "log_prob", "next_obs", "reward", "done", "terminal_obs")})]
    return out + ([("tracker.observe", b["done"], N)] if tracker else [])


def whole_rollout(K: int, *, tracker: bool) -> list[tuple]:
    KN = K * N
    return [("mlp.rollout_run", "env", ("obs_buf", 0, (T + 1, KN, W)),
             {"noise": ("noise_all", 0, (T, KN, A)), "value": ("val_buf", 0, (T, KN)), "action": ("act_buf", 0, (T, KN, A)),
              "log_prob": ("logp_buf", 0, (T, KN)), "reward": ("rew_buf", 0, (T, KN)), "done": ("done_buf", 0, (T, KN)),
              "terminal_obs": ("term_obs_buf", 0, (T, KN, W)), "first_step": 0, "n_steps": T, "trackers": "tracker" if tracker else None,
              "steps_per_call": N})]


def rollout_tail(p, *, monitor: bool = False, chunks: tuple = (CAP,)) -> list[tuple]:
    """_post_rollout: [monitor observe,] the bootstrap's critic forward (K = 1: in chunks of max_batch), the last value, the GAE scan,
    [the explained variance]"""
    K, KN = p.K, p.K * N
    out = [("monitor.observe", ("rew_buf", 0, (T, KN)), ("done_buf", 0, (T, KN)), T)] if monitor else []
    if isinstance(p, kpop.PopulationPPO):
        out.append(("mlp.forward", tmp((K * CAP, W), F32, 0, (K * CAP, W)), {"value": tmp((K * CAP,), F32, 0, (K * CAP,))}))
    else:
        s0 = 0
        for c in chunks:
            out.append(("mlp.forward", tmp((CAP, W), F32, s0 * W, (c, W)), {"value": tmp((CAP,), F32, s0, (c,))}))
            s0 += c
    out.append(("mlp.forward", ("obs_buf", T * KN * W, (KN, W)), {"value": tmp((KN,), F32, 0, (KN,))}))
    ptrs = [(name, 0) for name in ("rew_buf", "val_buf", "done_buf")] + [tmp((KN,), F32)]
    if getattr(p, "has_overrides", False):
        out.append(("kp1_gae_scan_replicas", 0, *ptrs, ("_gamma_lambda", 0), N, ("adv_buf", 0), ("ret_buf", 0), T, KN, "stream"))
    else:
        out.append(("kp1_gae_scan", 0, *ptrs, p.cfg.gamma, p.cfg.gae_lambda, ("adv_buf", 0), ("ret_buf", 0), T, KN, "stream"))
    if monitor:
        out.append(("kp1_explained_variance", 0, ("val_buf", 0), ("ret_buf", 0), T, KN, N, ("_ev_dev", 0), "stream"))
    return out


def minibatches(total: int, bs: int) -> list[tuple[int, int]]:
    return [(s0, min(s0 + bs, total) - s0) for s0 in range(0, total, bs)]


def epoch(p, *, normalize: bool = True) -> list[tuple]:
    """_epoch_body: the advantage statistics of every minibatch, then loss_grad [+ the gradient all-reduce] + adam_step per minibatch"""
    cfg, K, world = p.cfg, p.K, p.dist.world_size
    total, KN, P = T * N, K * N, p.flat.shape[-1]
    bs = max(cfg.batch_size // world, 1)
    mbs = minibatches(total, bs)
    n_mb = len(mbs)
    pop = isinstance(p, kpop.PopulationPPO)
    out = []
    if normalize and pop:
        for k in range(K):
            out.append(("kp1_adv_minibatch_sums", 0, ("adv_buf", 0), tmp((K, total), I64, k * total), total, bs, tmp((K, n_mb, 3), F64, k * n_mb * 3), "stream"))
        out.append(("kp1_adv_minibatch_stats", 0, tmp((K, n_mb, 3), F64), K * n_mb, tmp((K, n_mb, 2), F32), "stream"))
    elif normalize:
        out.append(("kp1_adv_minibatch_sums", 0, ("adv_buf", 0), ("perm", 0), total, bs, tmp((n_mb, 3), F64), "stream"))
        if world > 1:
            out.append(("dist.all_reduce_sum", tmp((n_mb, 3), F64, 0, (n_mb, 3))))
        out.append(("kp1_adv_minibatch_stats", 0, tmp((n_mb, 3), F64), n_mb, tmp((n_mb, 2), F32), "stream"))
    flat_shape = (K, P) if pop else (P,)
    for i, (s0, n) in enumerate(mbs):
        idx = tmp((K * total,), I64, K * s0, (K * n,)) if pop else ("perm", s0, (n,))
        # [n_mb][K][2], made contiguous from [K][n_mb][2] (K = 1: that already is, and no copy is made)
        stats = None if not normalize else tmp((n_mb, K, 2) if K > 1 else (1, n_mb, 2), F32, i * K * 2, (K, 2)) if pop else tmp((n_mb, 2), F32, i * 2, (2,))
        out.append(("mlp.loss_grad", ("obs_buf", 0, (T * KN, W)), idx, n, ("act_buf", 0, (T * KN, A)), ("logp_buf", 0, (T * KN,)),
                    ("adv_buf", 0, (T * KN,)), ("ret_buf", 0, (T * KN,)),
                    {"clip_range": cfg.clip_range, "ent_coef": cfg.ent_coef / world, "vf_coef": cfg.vf_coef, "inv_count": 1.0 / (n * world),
                     "grad_out": ("grad", 0, flat_shape), "stats_out": ("stats_dev", 0, (K, 4)), "adv_stats": stats, "normalize": normalize}))
        if world > 1:
            out.append(("dist.all_reduce_sum", ("grad", 0, flat_shape)))
        out.append(("mlp.adam_step", ("flat", 0, flat_shape), ("grad", 0, flat_shape), ("adam_m", 0, flat_shape), ("adam_v", 0, flat_shape),
                    {"lr": cfg.learning_rate, "eps": cfg.adam_eps, "max_grad_norm": cfg.max_grad_norm, "step": 0, "fused_norm": world == 1}))
    return out


def make(rec: _Rec, kind: str, **kw):
    p = {"ppo": lambda: _ppo(rec, **kw), "ppo_dp": lambda: _ppo(rec, world=2, **kw), "k_handle_1": lambda: _k_handle(rec, 1, **kw),
         "k_handle_2": lambda: _k_handle(rec, 2, **kw), "approach_1": lambda: _approach(rec, 1, **kw), "approach_2": lambda: _approach(rec, 2, **kw),
         "approach_2_overrides": lambda: _approach(rec, 2, overrides=True, **kw)}[kind]()
    return p


KINDS = ("ppo", "ppo_dp", "k_handle_1", "k_handle_2", "approach_1", "approach_2", "approach_2_overrides")


def handles(p, tracker: bool) -> dict[str, list[str]]:
    """the names of the env handles a step steps and of the trackers it observes"""
    if type(p) is kpop.PopulationPPO:
        return {"envs": [f"env{k}" for k in range(p.K)], "trackers": [f"tracker{k}" for k in range(p.K)] if tracker else []}
    return {"envs": ["env"], "trackers": ["tracker"] if tracker else []}


# ------------------------------------------------------------------------------------------------------------------------ construction
@pytest.mark.parametrize("kind", KINDS)
def test_construction(rec, kind):
    p = make(rec, kind, tracker=True, monitor=kind != "ppo_dp")
    K, pop, one = p.K, isinstance(p, kpop.PopulationPPO), isinstance(p, kpop.OneHandlePopulationPPO)
    h = handles(p, True)
    want = [("tracker.attach", "env")] if one else []
    if one:
        want += [("env.set_obs_stride", W)]                    # the views forward a change only: once for K views
    else:
        for env, cur in zip(h["envs"], h["trackers"]):
            want += [(f"{cur}.attach", env), (f"{env}.set_obs_stride", W)]
    max_batch = max(N, p.cfg.batch_size // p.dist.world_size, CAP if pop else 8192)
    want += [("mlp.create", 64, max_batch, 56, K), ("mlp.pack", ("flat", 0, tuple(p.flat.shape)))]
    if kind != "ppo_dp":
        want += [("monitor.create", K, N, 100, T), ("monitor.observe", ("rew_buf", 0, (T, K * N)), ("done_buf", 0, (T, K * N)), 1), ("monitor.reset_carry",),
                 ("kp1_explained_variance", 0, ("val_buf", 0), ("ret_buf", 0), T, K * N, N, ("_ev_dev", 0), "stream")]
    if kind == "approach_2_overrides":
        rows = [{f: getattr(c, f) for f in _Mlp.HPARAM_FIELDS} for c in p.cfgs]
        assert rows[0]["learning_rate"] == 1e-3 and rows[1]["learning_rate"] == 5e-4
        want += [("mlp.set_replica_hparams", rows)]
        assert p._gamma_lambda.tolist() == torch.tensor([[0.9, 0.95], [0.8, 0.95]]).tolist()
    assert rec.take() == want
    assert p.flat.shape == ((K, p.policies[0].numel) if pop else (p.policies[0].numel,)) and p.policies[0].flat.data_ptr() == p.flat.data_ptr()
    assert p.obs_buf.shape == (T + 1, K * N, W) and p.perm.shape == (K, T * N) and p.stats_dev.shape == (K, 4)
    if pop:
        assert p._trunc_cap == CAP
    if kind == "ppo_dp":
        assert p.done_chunk == 4 and p._done_gather.shape == (2, 4, N) and p._record_stage is None


# ------------------------------------------------------------------------------------------------------------------------ rollout steps, rollouts
FORMS = [(kind, form, tracker) for kind in KINDS for form in ("sequence", "fused", "whole") for tracker in (False, True)
         if not (form != "sequence" and kind in ("ppo_dp", "k_handle_1", "k_handle_2")) or (kind == "ppo_dp" and form == "fused")]


def _set_form(monkeypatch, form: str) -> None:
    monkeypatch.setenv("KP1_FUSED_ROLLOUT", "0" if form == "sequence" else "1")
    if form == "whole":
        monkeypatch.setenv("KP1_ROLLOUT_RUN", "1")


@pytest.mark.parametrize("kind, form, tracker", FORMS)
def test_rollout_step_and_rollout(rec, monkeypatch, kind, form, tracker):
    """one _rollout_step_hip(t) and one collect_rollouts() in each form the class can take: the launch sequence, the one-launch step
    (KP1_FUSED_ROLLOUT=1), the whole-rollout launch (KP1_ROLLOUT_RUN=1, ApproachPopulationPPO and PPO)"""
    _set_form(monkeypatch, form)
    p = make(rec, kind, tracker=tracker)
    rec.take()
    K, h = p.K, handles(p, tracker)
    k_handle = type(p) is kpop.PopulationPPO
    assert k_handle or p._fused_env_step == (form != "sequence")       # (the K-handle population steps its handles itself and never asks)
    assert bool(p._whole_rollout) == (form == "whole")

    def step(t: int) -> list[tuple]:
        if form == "sequence" or k_handle:
            out = launch_sequence_step(t, K, **h)
        else:
            out = fused_step(t, K, tracker=tracker)
        if kind == "ppo_dp" and tracker:         # the done bytes of a chunk of 4 steps are exchanged once, after its last step
            out = out[:-1]
            if (t + 1) % 4 == 0:
                out += [("dist.all_gather_into", ("_done_gather", 0, (2, 4, N)), ("done_buf", (t - 3) * N, (4, N))),
                        ("tracker.observe_chunk", ("_done_gather", 0, (2, 4, N)), N, 4, 2)]
        return out

    p._rollout_step_hip(2)
    assert rec.take() == step(2)
    resets = [(f"{env}.reset",) for env in h["envs"]]
    body = whole_rollout(K, tracker=tracker) if form == "whole" else [c for t in range(T) for c in step(t)]
    p.collect_rollouts()
    assert rec.take() == resets + body + rollout_tail(p)
    assert p.num_timesteps == T * N * p.dist.world_size and p._kernels_warm and not p._needs_reset
    p.collect_rollouts()                          # the second rollout starts where the first ended: no reset
    assert rec.take() == body + rollout_tail(p)

    seen = []
    p.step_callback = lambda done: seen.append(rec._item(done))          # a host hook after every step: the per-step loop, never the whole rollout
    p.collect_rollouts()
    want = [c for t in range(T) for c in step(t)] + rollout_tail(p)
    assert rec.take() == want and seen == [step_buffers(t, K * N)["done"] for t in range(T)]
    assert not p._whole_rollout


def test_rollout_forms_read_their_variable_first(rec, monkeypatch):
    """unset or "0", KP1_ROLLOUT_RUN / KP1_FUSED_ROUTE_ROLLOUT decide before the env is touched"""
    p = make(rec, "approach_2")
    p.pop_env = None                               # touching it would raise
    for value in (None, "0"):
        if value is not None:
            monkeypatch.setenv("KP1_ROLLOUT_RUN", value)
            monkeypatch.setenv("KP1_FUSED_ROUTE_ROLLOUT", value)
        assert p._whole_rollout is False and p._fused_route_step is False
    monkeypatch.setenv("KP1_ROLLOUT_RUN", "1")
    with pytest.raises(AttributeError):
        p._whole_rollout
    assert kpop.PopulationPPO._whole_rollout is False and kpop.ApproachPopulationPPO._whole_rollout is kppo.PPO._whole_rollout
    assert kpop.OneHandlePopulationPPO._policy_env_step is kppo.PPO._policy_env_step
    assert kpop.OneHandlePopulationPPO._curriculum_observe is kppo.PPO._curriculum_observe
    assert issubclass(kpop.OneHandlePopulationPPO, kpop.PopulationPPO) and issubclass(kpop.PopulationPPO, kppo.PPO)


# ------------------------------------------------------------------------------------------------------------------------ the rollout tail
def _truncations(p) -> dict[tuple[int, int], int]:
    """done bytes with truncations (2), terminations (1) and a truncated success (6: bit 1 set, bits 0-1 == 2); -> {(t, column): replica}
    of the truncated steps"""
    KN = p.K * N
    done = torch.zeros((T, KN), dtype=torch.uint8)
    where = {}
    for k in range(p.K):
        for t, n, byte in ((1, 0, 2), (3, 2, 6), (3, 1, 2), (0, 1, 1), (2, 2, 5)):
            done[t, k * N + n] = byte
            if byte & 3 == 2:
                where[(t, k * N + n)] = k
    done[1, 0] = 2 if p.K == 1 else 0               # replica 0 of a population has one truncation fewer: the counts differ per replica
    if p.K > 1:
        del where[(1, 0)]
    p.done_buf.copy_(done)
    return where


@pytest.mark.parametrize("kind, monitor", [(kind, monitor) for kind in KINDS for monitor in (False, True) if not (kind == "ppo_dp" and monitor)])
def test_post_rollout(rec, kind, monitor):
    """(a data-parallel run refuses the monitor: no such case)"""
    p = make(rec, kind, monitor=monitor)
    rec.take()
    where = _truncations(p)
    p._post_rollout()
    assert rec.take() == rollout_tail(p, monitor=monitor)
    # the critic's VALUE, discounted by the replica's gamma, went into the rewards of exactly the truncated steps
    gammas = [c.gamma for c in getattr(p, "cfgs", [p.cfg])]
    want = torch.zeros((T, p.K * N))
    for (t, col), k in where.items():
        want[t, col] = torch.tensor(gammas[k], dtype=torch.float32) * _Mlp.VALUE
    assert torch.equal(p.rew_buf, want)
    if monitor:                                    # the capture warm-up's tail feeds no episode data
        p._monitor_live = False
        p._post_rollout()
        assert rec.take() == rollout_tail(p, monitor=True)[1:]


def test_ppo_bootstrap_runs_the_critic_in_chunks_of_max_batch(rec, monkeypatch):
    monkeypatch.setattr(kmlp.MlpKernels, "max_batch_cap", 4)
    p = make(rec, "ppo")
    rec.take()
    _truncations(p)
    p._post_rollout()
    assert rec.take() == rollout_tail(p, chunks=(4, 4, 1))


# ------------------------------------------------------------------------------------------------------------------------ train()
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("batch_size", [4, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_train(rec, kind, batch_size, normalize):
    """n_epochs 2: per epoch the shuffles are drawn, the step count is set (eager, ungated) and the epoch body runs.  Batch size 5 splits
    the 12 rows into 5, 5, 2 (data parallel, 2 ranks: batch size 4 -> 2 rows per rank, 5 -> 2 as well)"""
    p = make(rec, kind, batch_size=batch_size, normalize_advantage=normalize, monitor=kind != "ppo_dp")
    rec.take()
    n_mb = len(minibatches(T * N, max(batch_size // p.dist.world_size, 1)))
    p.train()
    one = epoch(p, normalize=normalize)
    assert len([c for c in one if c[0] == "mlp.loss_grad"]) == n_mb == p._n_minibatches()
    assert rec.take() == [("mlp.set_step_count", 0)] + one + [("mlp.set_step_count", n_mb)] + one
    assert p.adam_t == 2 * n_mb and p.n_train_calls == 1
    for k in range(p.K):                           # every epoch drew a permutation of the replica's rows
        assert sorted(p.perm[k].tolist()) == list(range(T * N))
    p.train()
    assert [c for c in rec.take() if c[0] == "mlp.set_step_count"] == [("mlp.set_step_count", 2 * n_mb), ("mlp.set_step_count", 3 * n_mb)]


@pytest.mark.parametrize("kind", ["ppo", "k_handle_2", "approach_2", "approach_2_overrides"])
def test_train_with_a_kl_target_and_a_schedule(rec, kind):
    """a KL target: the gate is set once, armed per train() call, and the step count is the device's (never set from the host).  A
    schedule: every train() call stores the replicas' values of that call first"""
    p = make(rec, kind, batch_size=5, target_kl=0.02)
    assert rec.take()[-1] == ("mlp.set_kl_gate", [0.02] * p.K)
    p.train()
    one = epoch(p)
    assert rec.take() == [("mlp.kl_gate_arm",)] + one + one

    p = make(rec, kind, batch_size=5, learning_rate_schedule={"end": 1e-5, "end_fraction": 0.5})
    rec.take()
    p.progress_remaining = 0.75
    p.train()
    cfgs = getattr(p, "cfgs", [p.cfg])
    rows = [{**{f: float(getattr(c, f)) for f in _Mlp.HPARAM_FIELDS}, "learning_rate": kppo.linear_schedule(c.learning_rate, 1e-5, 0.5, 0.75)} for c in cfgs]
    assert rows[0]["learning_rate"] == 1e-3 + 0.25 * (1e-5 - 1e-3) / 0.5
    one = epoch(p)
    assert rec.take() == [("mlp.hparams_store", rows), ("mlp.set_step_count", 0)] + one + [("mlp.set_step_count", 3)] + one


def test_private_methods_other_callers_use(rec):
    """bench.py and the tools call ``_epoch_adv_stats(adv, perm, total, local_bs)`` with a 1-D perm, index the result ``[j]`` and pass it
    as ``adv_stats`` to ``_hip_minibatch_step(obs, idx, act, old_logp, adv, ret, device_step=True, adv_stats=...)``"""
    p = make(rec, "ppo", batch_size=5)
    rec.take()
    total = T * N
    obs, act = p.obs_buf[:T].view(total, W), p.act_buf.view(total, A)
    old_logp, adv, ret = p.logp_buf.view(total), p.adv_buf.view(total), p.ret_buf.view(total)
    perm = p.perm[0]
    stats = p._epoch_adv_stats(adv, perm, total, 5)
    assert stats.shape == (3, 2) and stats.dtype == torch.float32
    p._hip_minibatch_step(obs, perm[5:10], act, old_logp, adv, ret, device_step=True, adv_stats=stats[1])
    want = epoch(p)
    assert rec.take() == want[:2] + want[4:6]
    p._hip_minibatch_step(obs, perm[5:10], act, old_logp, adv, ret)          # device_step off: the host count goes up and is the step
    assert p.adam_t == 1 and rec.take()[-1][-1]["step"] == 1
    p.cfg.normalize_advantage = False
    assert p._epoch_adv_stats(adv, perm, total, 5) is None and rec.take() == []


# ------------------------------------------------------------------------------------------------------------------------ aten operations
# as recorded on the tree before section 46 (names without their ``aten.`` prefix)
POST_ROLLOUT_OPS = {
    "ppo": [
        "view.default", "bitwise_and.Scalar", "eq.Scalar", "nonzero_static.default", "view.default", "arange.default", "detach.default",
        "sum.default", "lt.Tensor", "view.default", "index_select.default", "empty.memory_format", "detach.default", "slice.Tensor", "slice.Tensor",
        "view.default", "mul.Tensor", "zeros_like.default", "detach.default", "where.self", "index_add_.default", "empty.memory_format",
        "detach.default", "select.int"],
    "approach_2": [
        "view.default", "permute.default", "bitwise_and.Scalar", "eq.Scalar", "clone.default", "_unsafe_view.default", "select.int",
        "nonzero_static.default", "view.default", "select.int", "nonzero_static.default", "view.default", "stack.default", "floor_divide.default",
        "mul.Tensor", "add.Tensor", "remainder.Scalar", "add.Tensor", "arange.default", "detach.default", "view.default", "sum.dim_IntList",
        "lt.Tensor", "view.default", "view.default", "index_select.default", "empty.memory_format", "detach.default", "mul.Tensor", "view.default",
        "view.default", "view.default", "zeros_like.default", "detach.default", "where.self", "index_add_.default", "empty.memory_format",
        "detach.default", "select.int"],
    "approach_2_overrides": [
        "view.default", "permute.default", "bitwise_and.Scalar", "eq.Scalar", "clone.default", "_unsafe_view.default", "select.int",
        "nonzero_static.default", "view.default", "select.int", "nonzero_static.default", "view.default", "stack.default", "floor_divide.default",
        "mul.Tensor", "add.Tensor", "remainder.Scalar", "add.Tensor", "arange.default", "detach.default", "view.default", "sum.dim_IntList",
        "lt.Tensor", "view.default", "view.default", "index_select.default", "empty.memory_format", "detach.default", "slice.Tensor", "view.default",
        "mul.Tensor", "view.default", "view.default", "view.default", "view.default", "zeros_like.default", "detach.default", "where.self",
        "index_add_.default", "empty.memory_format", "detach.default", "select.int"],
}
_POPULATION_EPOCH_OPS = [
    "slice.Tensor", "view.default", "view.default", "view.default", "view.default", "view.default", "floor_divide.default", "mul.Tensor",
    "add.Tensor", "remainder.Scalar", "add.Tensor", "view.default", "index_select.default", "empty.memory_format", "detach.default", "select.int",
    "select.int", "select.int", "select.int", "empty.memory_format", "detach.default", "permute.default", "clone.default", "slice.Tensor",
    "select.int", "slice.Tensor", "select.int", "slice.Tensor", "select.int"]
EPOCH_BODY_OPS = {
    "ppo": [
        "slice.Tensor", "view.default", "view.default", "view.default", "view.default", "view.default", "select.int", "empty.memory_format",
        "detach.default", "empty.memory_format", "detach.default", "slice.Tensor", "select.int", "slice.Tensor", "select.int", "slice.Tensor",
        "select.int"],
    "approach_2": _POPULATION_EPOCH_OPS,
    "approach_2_overrides": _POPULATION_EPOCH_OPS,       # the kernels read the table: Python does the same
}


@pytest.mark.parametrize("kind", ["ppo", "approach_2", "approach_2_overrides"])
def test_aten_operations_of_the_tail_and_the_epoch(rec, kind):
    """the aten operations ``_post_rollout()`` and ``_epoch_body()`` issue, views included, as the tree before section 46 issued them: each
    elementwise one is a launch per replay of the captured rollout and epoch graphs"""
    p = make(rec, kind, batch_size=5)
    _truncations(p)
    rec.take_ops()
    p._post_rollout()
    assert rec.take_ops() == POST_ROLLOUT_OPS[kind]
    p._epoch_body()
    assert rec.take_ops() == EPOCH_BODY_OPS[kind]
