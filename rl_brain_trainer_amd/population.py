"""Population PPO: K independent seeds trained at once through ONE launch sequence of the layer-wise MLP kernels.

The reference copes with its seed-fragile training at reference scale (16 envs x 1024 steps, minibatch 256, 2x64) by selecting checkpoints
across seeds (best-by-gate, train_workspace_expansion.py:54-129).  At that scale every kernel of an optimiser step covers a handful of
workgroups, so a step costs about its launch count; a population handle (include/kp1_ppo.h, kp1_mlp_create_population) puts the replica on
a grid axis and K seeds then cost about the launches of one.

Replica k of a population is bit-identical to ``PPO(seed=s_k)`` on the same config (tests/test_population_gpu.py):

* one env handle per replica, ``env_factory(s_k)`` -- the env step kernel, its reset sampler and the tracker's device stage are unchanged --
  stepped into row slice [k N, (k + 1) N) of rollout buffers laid out [T(+1), K N, ...]; GAE and the bootstrap run per column, so one launch
  covers all replicas;
* each replica owns the generators a single PPO owns (ActorCritic init, rollout noise, minibatch shuffles) and its own tracker;
* a replica's minibatch index p in [0, T N) maps to the global row t K N + k N + n; the kernels keep each replica's reduction order and
  chunking (the per-replica minibatch geometry is a single run's), and all replicas share one Adam step count.

The one-handle forms (``ApproachPopulationPPO``, ``RoutePopulationPPO``) step all replicas in ONE env handle of K N envs instead, block k
being replica k, with one population tracker: every env step is one env launch and one tracker launch whatever K is.

``PopulationPPO`` is a ``PPO`` with K replicas: it runs PPO's rollout, graph capture, rollout tail, optimiser step and update loop and
overrides only the steps that depend on K.  ``replica(k)`` is a view with what ``checkpoint.save`` and the evaluators read, so a replica
saves as an ordinary single-policy archive.
"""
from __future__ import annotations

import dataclasses
from typing import Any, Callable

import torch

from . import native
from .curriculum import PointCurriculumPopulation
from .finisher_tools import DockReverseCurriculumPopulation
from .ppo import ACT_DIM, OBS_DIM, Dist, PPO, PPOConfig, check_schedules, check_target_kl, truncation_cap
from .route_curriculum import RoutePrefixCurriculumPopulation
from .route_env import RoutePopulationVecEnv
from .vec_env import ArmKinematicPopulationVecEnv

MAX_REPLICAS = native.header_int("KP1_MLP_MAX_REPLICAS")

# Per-replica PPO hyper-parameters a population can sweep (``overrides``): the six the MLP kernels read from the handle's table
# (kp1_mlp_set_replica_hparams), the two of the per-replica GAE scan / bootstrap, and target_kl, which reaches the handle as the [K] target
# array of its KL gate (kp1_mlp_set_kl_gate) and is the one key that also takes None ("none": no early stop for that replica).  The
# geometry the replicas share is refused.
SWEEPABLE = ("learning_rate", "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "adam_eps", "gamma", "gae_lambda", "target_kl")
NONE_WORDS = ("none", "null", "off")     # target_kl=none
SHAPE_KEYS = ("n_steps", "batch_size", "n_epochs", "hidden", "normalize_advantage")


def check_overrides(seeds: list[int], overrides: list[dict[str, float]] | None) -> list[dict[str, float]]:
    """The host-side refusals of per-replica overrides (before any device work): one dict per replica, sweepable keys only, finite values,
    distinct (seed, overrides) pairs.  Returns the overrides as {key: float} dicts ([{}] * K when None)."""
    import math

    K = len(seeds)
    if overrides is None:
        out: list[dict[str, float]] = [{} for _ in range(K)]
    else:
        if len(overrides) != K:
            raise ValueError(f"{len(overrides)} override dicts for {K} replicas: a population takes one per replica")
        out = []
        for k, o in enumerate(overrides):
            row: dict[str, float] = {}
            for key, v in dict(o).items():
                if key == "seed":
                    raise ValueError("overrides cannot set 'seed': a replica's seed is its entry of the seed list")
                if key in SHAPE_KEYS:
                    raise ValueError(f"overrides cannot set {key!r}: the replicas of a population share the rollout and minibatch geometry "
                                     f"({', '.join(SHAPE_KEYS)})")
                if key not in SWEEPABLE:
                    raise ValueError(f"unknown override {key!r} (sweepable: {', '.join(SWEEPABLE)})")
                if key == "target_kl" and (v is None or (isinstance(v, str) and v.strip().lower() in NONE_WORDS)):
                    row[key] = None
                    continue
                if isinstance(v, bool):
                    raise ValueError(f"override {key}={v!r} of replica {k} is not a number")
                try:
                    fv = float(v)
                except (TypeError, ValueError) as exc:
                    raise ValueError(f"override {key}={v!r} of replica {k} is not a number") from exc
                if not math.isfinite(fv):
                    raise ValueError(f"override {key}={v!r} of replica {k} is not finite")
                if key == "target_kl" and fv <= 0.0:
                    raise ValueError(f"override target_kl={v!r} of replica {k} must be positive (or none)")
                row[key] = fv
            out.append(row)
    pairs = [(s, tuple(sorted(o.items(), key=lambda kv: kv[0]))) for s, o in zip(seeds, out)]
    if len(set(pairs)) != len(pairs):
        raise ValueError(f"(seed, overrides) pairs must be distinct (seeds {list(seeds)}, overrides {out}): equal pairs train identical replicas")
    return out


class _ReplicaDist:
    enabled, world_size, rank = False, 1, 0


class ReplicaView:
    """Replica k of a PopulationPPO, with the attributes ``checkpoint.save`` and the evaluators read from a PPO."""

    def __init__(self, pop: "PopulationPPO", k: int) -> None:
        self._pop, self.k = pop, k
        self.cfg = pop.cfgs[k]
        self.seed = pop.seeds[k]
        self.policy = pop.policies[k]
        self.adam_m = pop.adam_m[k]
        self.adam_v = pop.adam_v[k]
        self.env = pop.envs[k]
        self.curriculum = pop.curricula[k]
        self.n_envs = pop.n_envs
        self.obs_dim = pop.obs_dim
        self.obs_w = pop.obs_w
        self.dist = _ReplicaDist()
        self.backend = "hip"
        self.device = pop.device

    adam_t = property(lambda self: self._pop.adam_step_count(self.k))     # the replica's own count where target_kl lets the replicas differ
    actor_extra_steps = property(lambda self: int(self._pop.actor_extra_steps))   # shared: every replica takes the same teacher-anchor steps
    num_timesteps = property(lambda self: self._pop.num_timesteps)
    n_train_calls = property(lambda self: self._pop.n_train_calls)
    last_stats = property(lambda self: self._pop.replica_stats(self.k))
    update_form = property(lambda self: self._pop.update_form)
    # a scheduled population: the shared schedules and clock, this replica's values of the last train() call
    hparam_schedules = property(lambda self: self._pop.hparam_schedules)
    progress_remaining = property(lambda self: self._pop.progress_remaining)

    def current_hparams(self, k: int = 0) -> dict[str, float]:
        """this replica's learning rate and clip range as the last train() call used them"""
        return self._pop.current_hparams(self.k)

    def n_updates(self, k: int = 0) -> int:
        """SB3's ``_n_updates`` of this replica"""
        return self._pop.n_updates(self.k)

    @torch.no_grad()
    def predict(self, obs: torch.Tensor, deterministic: bool = True) -> torch.Tensor:
        """model.predict(obs, deterministic=True): mean action clipped to the action space"""
        if not deterministic:
            raise NotImplementedError("a population replica predicts deterministically (evaluators use deterministic=True)")
        return self._pop.infer_policy(self.k).predict(obs)


def _per_replica(name: str):
    """a PPO method that acts on one policy: refused on a population, whose K policies are reached through replica(k) / infer_policy(k)"""

    def refuse(self, *args, **kwargs):
        raise TypeError(f"PopulationPPO.{name}: a population holds {self.K} policies; use replica(k) (checkpoint.save, the evaluators, "
                        "last_stats) or infer_policy(k) (predict)")

    return refuse


class PopulationPPO(PPO):
    """K = len(seeds) PPO runs of one PPOConfig, trained together.  ``env_factory(seed)`` builds replica k's env handle (first env id 0);
    ``curriculum_factory(seed)`` (optional) its PointCurriculum / DockReverseCurriculum, attached to that handle.

    PPO's rollout, graph capture, rollout tail, optimiser step and update loop run unchanged on K replicas; what depends on K is overridden
    here: the env step and the tracker per replica slice, the per-replica compacted bootstrap, the noise draw from each replica's generator,
    the GAE scan where overrides give the replicas their own (gamma, lambda), and the index preparation of the epoch body, which hands
    PPO's optimiser step minibatch i of every replica as one [K][n] index block (``_global_rows``: the one replica-major row mapping)."""

    def __init__(self, seeds: list[int], cfg: PPOConfig, env_factory: Callable[[int], Any], *,
                 curriculum_factory: Callable[[int], Any] | None = None, dist: Dist | None = None, use_graphs: bool = True,
                 teacher_anchor: Any = None, overrides: list[dict[str, float]] | None = None, monitor: bool | int = False) -> None:
        seeds, dist, overrides = self._check_population_args(seeds, cfg, dist, teacher_anchor, overrides)
        envs: list[Any] = []
        try:
            for s in seeds:
                env = env_factory(s)
                envs.append(env)
                if int(getattr(env, "obs_dim", OBS_DIM)) != OBS_DIM:
                    raise ValueError("PopulationPPO takes the 56-float ArmKinematicEnv observation; route envs (obs_dim 80) are not supported")
                if env.dtype != torch.float32:
                    raise ValueError("PopulationPPO drives the production f32 env")
            if len({e.n_envs for e in envs}) != 1:
                raise ValueError("every replica's env must have the same number of envs")
        except BaseException:
            for e in envs:
                e.close()
            raise
        curricula = [curriculum_factory(s) if curriculum_factory is not None else None for s in seeds]
        self._init_population(seeds, cfg, envs, curricula, dist, use_graphs, overrides, monitor=monitor)

    @staticmethod
    def _check_population_args(seeds: list[int], cfg: PPOConfig, dist: Dist | None, teacher_anchor: Any,
                               overrides: list[dict[str, float]] | None = None, *,
                               accepts_anchor: bool = False) -> tuple[list[int], Dist, list[dict[str, float]]]:
        """the refusals every population shares; returns (seeds as ints, the Dist, the per-replica overrides).  ``accepts_anchor``: a
        PopulationTeacherAnchor passes (RoutePopulationPPO); anything else given as ``teacher_anchor`` is refused"""
        seeds = [int(s) for s in seeds]
        if not seeds:
            raise ValueError("PopulationPPO needs at least one seed")
        if len(seeds) > MAX_REPLICAS:
            raise ValueError(f"PopulationPPO trains at most {MAX_REPLICAS} replicas at once (got {len(seeds)} seeds)")
        overrides = check_overrides(seeds, overrides)
        if cfg.hidden not in (64, 128):
            raise ValueError(f"PopulationPPO runs the layer-wise kernels of the 2x64 / 2x128 nets; hidden={cfg.hidden} is not supported "
                             "(the 2x256 tile kernels have no replica axis)")
        if teacher_anchor is not None:
            from .teacher_anchor import PopulationTeacherAnchor

            if not accepts_anchor:
                raise ValueError("this population does not support the teacher-anchor side loss: it is a route feature "
                                 "(RoutePopulationPPO with a PopulationTeacherAnchor)")
            if not isinstance(teacher_anchor, PopulationTeacherAnchor):
                raise ValueError("the teacher-anchor side loss of a route population is a PopulationTeacherAnchor "
                                 f"(got {type(teacher_anchor).__name__}; RouteTeacherAnchor steps one PPO)")
        dist = dist or Dist()
        if dist.enabled:
            raise ValueError("PopulationPPO is single-process: data parallel (a torch.distributed process group) is not supported")
        check_target_kl([o.get("target_kl", cfg.target_kl) for o in overrides], dist, teacher_anchor)
        check_schedules(cfg, teacher_anchor)
        return seeds, dist, overrides

    def _init_population(self, seeds: list[int], cfg: PPOConfig, envs: list[Any], curricula: list[Any], dist: Dist, use_graphs: bool,
                         overrides: list[dict[str, float]] | None = None, *, min_batch: int = 0, monitor: bool | int = False) -> None:
        """what a population holds once its K env views and trackers exist (``min_batch``: rows the MLP handle must hold besides its own needs)"""
        T, N, K = cfg.n_steps, envs[0].n_envs, len(seeds)
        self._trunc_cap = truncation_cap(T, N, envs[0])
        # the MLP handle's max_batch holds the `_trunc_cap` rows per replica of the bootstrap's one forward
        self._setup(cfg, seeds, envs, curricula, dist, use_graphs, min_batch=max(self._trunc_cap, int(min_batch)), stacked=True, monitor=monitor)
        self.seeds = seeds
        self.overrides = overrides if overrides is not None else [{} for _ in seeds]
        # a population with overrides keeps its per-replica constants on the device: the MLP handle's hyper-parameter table, (gamma, lambda)
        # per replica for the GAE scan and gamma per replica for the bootstrap.  Captured graphs hold their addresses, so the values are
        # refreshed in place (_apply_overrides) and never re-allocated.
        self.has_overrides = any(self.overrides)
        dev = self.device
        self._gamma_lambda = torch.zeros((K, 2), dtype=torch.float32, device=dev) if self.has_overrides else None
        self._apply_overrides()
        self._setup_kl_gate(check_target_kl([c.target_kl for c in self.cfgs], dist))
        # every replica anneals from its own start (cfgs[k].learning_rate / clip_range: the sweep's value) to the shared end
        self._setup_schedules(check_schedules(cfg))
        self.noise_rep = torch.zeros((K, T, N, ACT_DIM), dtype=torch.float32, device=dev)   # replica k's draw, as PPO.noise_all
        # minibatch i of replica k = local positions [start_i, end_i) of its shuffle; the kernels read minibatch i as ONE [K][n_i] index
        # block at K * start_i of the gathered index vector
        total, bs = T * N, max(cfg.batch_size, 1)
        self._mb = [(s0, min(s0 + bs, total)) for s0 in range(0, total, bs)]
        src = [k * total + torch.arange(s0, e0) for s0, e0 in self._mb for k in range(K)]
        self._mb_src = torch.cat(src).to(dev)
        self._rep_off = (torch.arange(K, device=dev, dtype=torch.int64) * N).view(K, 1)
        self._infer: dict[int, Any] = {}

    def _global_rows(self, loc: torch.Tensor) -> torch.Tensor:
        """[K, n] positions p in [0, T N) of each replica's own rollout (row k: replica k's) -> rows of the [T, K N] buffers: step p // N,
        column k N + p % N"""
        N = self.n_envs
        return (loc // N) * (self.K * N) + self._rep_off + loc % N

    def _apply_overrides(self) -> None:
        """cfgs[k] = cfg with replica k's seed and overrides; a population with overrides writes them to the device (at construction and
        after load_init_checkpoints, always before the first capture)"""
        self.cfgs = [dataclasses.replace(self.cfg, seed=s, **o) for s, o in zip(self.seeds, self.overrides)]
        if not self.has_overrides:
            return
        self._mlp.set_replica_hparams([{f: getattr(c, f) for f in self._mlp.HPARAM_FIELDS} for c in self.cfgs])
        self._gamma_lambda.copy_(torch.tensor([[c.gamma, c.gae_lambda] for c in self.cfgs], dtype=torch.float32))

    # ------------------------------------------------------------------ views
    def replica(self, k: int) -> ReplicaView:
        return ReplicaView(self, k)

    @property
    def replica_names(self) -> list[str]:
        """replica_name of every replica: its artefact directory, and what ppo.run_training calls it above its monitor record"""
        return [replica_name(s, o) for s, o in zip(self.seeds, self.overrides)]

    def close(self) -> None:
        for e in self.envs:
            e.close()
        self._mlp.close()
        if self.monitor is not None:
            self.monitor.close()

    def infer_policy(self, k: int):
        """a K = 1 inference handle on replica k's current parameters (for predict / the evaluators)"""
        from .ppo import InferencePolicy

        pol = self._infer.get(k)
        if pol is None:
            pol = self._infer[k] = InferencePolicy(self.policies[k].state_dict(), device=self.device)
        else:
            pol.policy.flat.copy_(self.flat[k])
            pol._mlp.pack(pol.policy.flat)
        return pol

    def replica_stats(self, k: int) -> dict[str, float]:
        """PPO.last_stats of replica k (reading it synchronises with the last update)"""
        return self._stats_rows()[k]

    predict = _per_replica("predict")
    predict_unclipped = _per_replica("predict_unclipped")
    load_checkpoint = _per_replica("load_checkpoint")
    last_stats = property(_per_replica("last_stats"))

    # ------------------------------------------------------------------ rollout
    # the whole-rollout form (kp1_rollout_run) steps ONE env handle: the K-handle population, and the dock and route one-handle populations,
    # keep the per-step loop; ApproachPopulationPPO takes PPO's predicate back
    _whole_rollout = False

    def _draw_noise(self) -> None:
        for k in range(self.K):
            self.noise_rep[k].normal_(generator=self.gens[k])
        self.noise_all.view(self.cfg.n_steps, self.K, self.n_envs, ACT_DIM).copy_(self.noise_rep.permute(1, 0, 2, 3))

    def _policy_env_step(self, t: int) -> None:
        self._mlp.forward(self.obs_buf[t], noise=self.noise_all[t], value=self.val_buf[t], action=self.act_buf[t], clipped=self.clip_act,
                          log_prob=self.logp_buf[t])
        for k, env in enumerate(self.envs):
            sl = self._sl(k)
            env.step_into(self.clip_act[sl], self.obs_buf[t + 1, sl], self.rew_buf[t, sl], self.done_buf[t, sl], self.term_obs_buf[t, sl], True)

    def _curriculum_observe(self, t: int) -> None:
        for k, cur in enumerate(self.curricula):
            if cur is not None:
                cur.observe(self.done_buf[t, self._sl(k)], self.n_envs)

    def _bootstrap_truncated(self) -> None:
        """PPO._bootstrap_truncated per replica: the critic of replica k on its (at most cap) truncated terminal observations"""
        K, T, N, cap = self.K, self.cfg.n_steps, self.n_envs, self._trunc_cap
        trunc = ((self.done_buf.view(T, K, N).permute(1, 0, 2) & 3) == 2).reshape(K, T * N)
        loc = torch.stack([torch.nonzero_static(trunc[k], size=cap, fill_value=0).view(-1) for k in range(K)])
        gidx = self._global_rows(loc)
        valid = torch.arange(cap, device=self.device).view(1, cap) < trunc.sum(dim=1, keepdim=True)
        sel = self.term_obs_buf.view(T * K * N, self.obs_w).index_select(0, gidx.view(-1))
        tv = torch.empty(K * cap, dtype=torch.float32, device=self.device)
        # one forward of `cap` rows per replica: the handle's max_batch is sized to hold them (min_batch in __init__), so unlike PPO nothing
        # is chunked here -- shrinking max_batch below _trunc_cap would make this call fail
        self._mlp.forward(sel, value=tv)
        # replica k's rows times replica k's gamma: the fp32 product of PPO's cfg.gamma * tv
        disc = self.cfg.gamma * tv if not self.has_overrides else (self._gamma_lambda[:, :1] * tv.view(K, cap)).view(-1)
        self.rew_buf.view(-1).index_add_(0, gidx.view(-1), torch.where(valid.view(-1), disc, torch.zeros_like(tv)))

    def _gae_scan(self, last_v: torch.Tensor) -> None:
        """with overrides the scan reads each replica's (gamma, lambda) (kp1_gae_scan_replicas, one launch)"""
        if not self.has_overrides:
            return super()._gae_scan(last_v)
        native.check(self.L.kp1_gae_scan_replicas(native.device_index(self.device), native.ptr(self.rew_buf), native.ptr(self.val_buf),
                                                  native.ptr(self.done_buf), native.ptr(last_v), native.ptr(self._gamma_lambda), self.n_envs,
                                                  native.ptr(self.adv_buf), native.ptr(self.ret_buf), self.cfg.n_steps, self.K * self.n_envs,
                                                  native.stream_arg(self.device)))

    # ------------------------------------------------------------------ update
    def _epoch_body(self) -> None:
        """one update epoch from the shuffles in self.perm: global row indices, minibatch i of every replica as one [K][n_i] index block, the
        per-replica minibatch advantage statistics, then PPO's optimiser step per minibatch"""
        cfg = self.cfg
        T = cfg.n_steps
        obs = self.obs_buf[:T].view(-1, self.obs_w)
        act = self.act_buf.view(-1, ACT_DIM)
        old_logp, adv, ret = self.logp_buf.view(-1), self.adv_buf.view(-1), self.ret_buf.view(-1)
        gperm = self._global_rows(self.perm)                                          # [K, T N] global rows
        mb_idx = gperm.view(-1).index_select(0, self._mb_src)
        stats = self._epoch_adv_stats(adv, gperm, T * self.n_envs, cfg.batch_size)
        for i, (s0, e0) in enumerate(self._mb):
            self._hip_minibatch_step(obs, mb_idx[self.K * s0:self.K * e0], act, old_logp, adv, ret, device_step=True,
                                     adv_stats=None if stats is None else stats[i])


class OneHandlePopulationPPO(PopulationPPO):
    """A population whose K replicas share ONE env handle of K N envs (block k = replica k, the rollout buffers' replica-major layout) and
    ONE population tracker: every env step is one env step launch and one tracker launch whatever K is.  The rollout step is PPO's own, on
    ``pop_env`` / ``pop_curriculum``; noise, truncation bootstrap, the epoch body and graph capture are PopulationPPO's.  A subclass names
    what it drives in the class attributes below.  The caller owns (and closes) the env and the tracker."""

    pop_env: Any = None
    pop_curriculum: Any = None

    # what __init__ checks, in the order of its refusals: the env class, a further predicate on the env with the words that name such an env,
    # the tracker class, whether the tracker's K must equal the seed count, whether a PopulationTeacherAnchor is accepted
    env_class: type = type(None)
    env_also = staticmethod(lambda env: True)
    env_words = ""
    tracker_class: type = type(None)
    tracker_checks_k = True
    accepts_anchor = False
    # whether the env handle is one kp1_mlp_forward_env_step steps (an ArmKinematicPopulationVecEnv; the route env has no kp1_env step of its
    # own and the 80-float observation, so RoutePopulationPPO keeps the launch sequence), and one kp1_mlp_forward_route_step steps
    fused_env_type_ok = False
    fused_route_env_type_ok = False

    def __init__(self, seeds: list[int], cfg: PPOConfig, env: Any, *, curriculum: Any = None, dist: Dist | None = None, use_graphs: bool = True,
                 teacher_anchor: Any = None, overrides: list[dict[str, float]] | None = None, monitor: bool | int = False) -> None:
        name, env_name, tracker_name = type(self).__name__, self.env_class.__name__, self.tracker_class.__name__
        seeds, dist, overrides = self._check_population_args(seeds, cfg, dist, teacher_anchor, overrides, accepts_anchor=self.accepts_anchor)
        if not isinstance(env, self.env_class) or not self.env_also(env):
            raise TypeError(f"{name} drives {self.env_words} (one handle for all replicas)")
        if env.seeds != seeds:
            raise ValueError(f"the {env_name} was made for seeds {env.seeds}, not {seeds}")
        if curriculum is not None and not isinstance(curriculum, self.tracker_class):
            raise TypeError(f"{name} takes a {tracker_name} (one tracker launch for all replicas)")
        if curriculum is not None and self.tracker_checks_k and curriculum.K != len(seeds):
            raise ValueError(f"the {tracker_name} holds {curriculum.K} trackers for {len(seeds)} seeds")
        self.pop_env, self.pop_curriculum = env, curriculum
        if curriculum is not None:
            curriculum.attach(env)
        K = len(seeds)
        views = [env.replica(k) for k in range(K)]
        curricula = [curriculum.replica(k) if curriculum is not None else None for k in range(K)]
        # with an anchor the MLP handle also holds one teacher-anchor batch per replica (PopulationTeacherAnchor steps it between rollout
        # and update)
        self._init_population(seeds, cfg, views, curricula, dist, use_graphs, overrides,
                              min_batch=teacher_anchor.batch_rows if teacher_anchor is not None else 0, monitor=monitor)
        self.teacher_anchor = teacher_anchor
        if teacher_anchor is not None:
            teacher_anchor.on_training_start(self)

    def _reset_envs(self, which: list[int] | None = None) -> None:
        if which is None or which:
            self.obs_buf[0].copy_(self.pop_env.reset())
            self._monitor_reset_carry()

    # PPO's rollout step (not the K-handle population's), on the one handle and the one tracker
    _policy_env_step = PPO._policy_env_step
    _curriculum_observe = PPO._curriculum_observe

    def _rollout_env(self) -> Any:
        return self.pop_env

    def _rollout_tracker(self) -> Any:
        return self.pop_curriculum

    def _rollout_env_type_ok(self) -> bool:
        return self.fused_env_type_ok

    def _route_env_type_ok(self) -> bool:
        return self.fused_route_env_type_ok

    def _fused_rollout_default(self) -> bool:
        return True     # measured on both one-handle trainers

    def _warm_curricula(self) -> None:
        if self.pop_curriculum is not None:
            self.pop_curriculum.observe(self.done_buf[0].zero_(), 0)

    @staticmethod
    def check_init_checkpoint(path: str) -> dict[str, int]:
        """refuse (on the host, before any device work) a checkpoint whose Adam state carries teacher-anchor actor steps; returns what a
        population must share with the other replicas' checkpoints: hidden width, Adam step count (0 without an Adam state), num_timesteps"""
        import math

        from . import checkpoint
        from .ppo import load_adam_state, param_spec

        hidden, obs_dim = (int(v) for v in checkpoint.load_policy_state_dict(path)["mlp_extractor.policy_net.0.weight"].shape)
        out = {"hidden": hidden, "adam_steps": 0}
        opt = checkpoint.load_optimizer_state_dict(path)
        if opt and opt.get("state"):
            spec = param_spec(hidden, obs_dim)
            n = sum(math.prod(shape) for _, shape in spec)
            adam_t, extra = load_adam_state(opt, spec, torch.zeros(n), torch.zeros(n))
            if extra:
                raise ValueError(f"{path} carries {extra} teacher-anchor actor steps (actor_extra_steps); a population keeps one Adam step "
                                 "count for every tensor and cannot resume it")
            out["adam_steps"] = int(adam_t)
        try:
            out["num_timesteps"] = int(checkpoint.load_data(path).get("num_timesteps", 0))
        except KeyError:        # an archive without SB3's data member (a bare policy + optimizer zip)
            out["num_timesteps"] = 0
        return out

    @classmethod
    def check_init_checkpoints(cls, paths: list[str]) -> dict[str, int]:
        """check_init_checkpoint of every replica's checkpoint, and the refusals of a per-replica start: the replicas must agree on the Adam
        step count and num_timesteps (a population shares one of each), and the width must be one a population trains (64 or 128)"""
        infos = [cls.check_init_checkpoint(p) for p in paths]
        for key, what in (("adam_steps", "Adam step counts"), ("num_timesteps", "num_timesteps"), ("hidden", "hidden widths")):
            values = sorted({i[key] for i in infos})
            if len(values) > 1:
                raise ValueError(f"the replicas' checkpoints differ in their {what} ({values}); a population shares one")
        if infos and infos[0]["hidden"] not in (64, 128):
            raise ValueError(f"the checkpoints hold a 2x{infos[0]['hidden']} policy; a population trains 2x64 or 2x128 nets")
        return infos[0] if infos else {}

    def load_init_checkpoint(self, path: str) -> dict[str, Any]:
        """``PPO.load_checkpoint(path, restore_timesteps=True, restore_hyperparameters=True)`` into every replica (train_route's
        --init-checkpoint, train_dock's --seeds --resume-from <zip>): weights, Adam moments, the Adam step count, the step clock and the
        saved algorithm constants; the learning rate stays the config's.  A checkpoint with teacher-anchor actor steps is refused: a
        population has one Adam step count for every tensor."""
        return self.load_init_checkpoints([path] * self.K)

    def load_init_checkpoints(self, paths: list[str], *, restore_timesteps: bool = True) -> dict[str, Any]:
        """the per-replica form: replica k starts from ``paths[k]`` (weights and Adam moments); the step count, the clock and the saved
        algorithm constants are shared, so check_init_checkpoints refuses checkpoints that disagree on them.  Per-replica overrides apply
        after the saved constants.  ``restore_timesteps=False`` keeps the step clock and the update count at zero, as train.py's
        ``PPO.load_checkpoint(restore_hyperparameters=True)`` does."""
        from . import checkpoint
        from .ppo import load_adam_state, restore_saved_hyperparameters

        if len(paths) != self.K:
            raise ValueError(f"{len(paths)} checkpoints for {self.K} replicas")
        if self.adam_t or self.n_train_calls or self._epoch_graph is not None:
            raise RuntimeError("load_init_checkpoint must happen before the first update")
        self.check_init_checkpoints(paths)
        restored: dict[str, Any] = {"policy": True, "optimizer": False}
        for k, path in enumerate(paths):
            if k > 0 and path == paths[0]:
                self.policies[k].load_state_dict(self.policies[0].state_dict())
                if restored["optimizer"]:
                    self.adam_m[k].copy_(self.adam_m[0])
                    self.adam_v[k].copy_(self.adam_v[0])
                continue
            self.policies[k].load_state_dict(checkpoint.load_policy_state_dict(path))
            opt = checkpoint.load_optimizer_state_dict(path)
            if opt and opt.get("state"):
                adam_t, _ = load_adam_state(opt, self.policies[k].spec, self.adam_m[k], self.adam_v[k])
                self.adam_t = adam_t
                restored.update({"optimizer": True, "adam_steps": adam_t, "actor_extra_steps": 0})
        self._mlp.pack(self.flat)
        self._mlp.set_step_count(self.adam_t)
        data = checkpoint.load_data(paths[0])
        if restore_timesteps:
            self.num_timesteps = int(data.get("num_timesteps", 0))
            restored["num_timesteps"] = self.num_timesteps
            saved_epochs = data.get("n_epochs")
            if isinstance(data.get("_n_updates"), int) and isinstance(saved_epochs, int) and saved_epochs > 0:
                self.n_train_calls = int(data["_n_updates"]) // saved_epochs
        restored["hyperparameters"] = restore_saved_hyperparameters(self.cfg, data)
        self._apply_overrides()     # swept values beat both the config and the checkpoint
        self._kl_after_load()
        return restored


class ApproachPopulationPPO(OneHandlePopulationPPO):
    """K Approach runs of one PPOConfig on ONE ArmKinematicPopulationVecEnv (vec_env.py) with ONE PointCurriculumPopulation
    (curriculum.py): the env step kernel reads each env's stage from its own replica's tracker, so replicas on different stages share a
    launch (and a wave).  Replica k is bit-identical to ``PPO(ArmKinematicVecEnv(..., seed=s_k), curriculum=PointCurriculum)`` on the same
    config (tests/test_approach_population_gpu.py), and to replica k of the K-handle ``PopulationPPO``."""

    env_class, env_words, tracker_class = ArmKinematicPopulationVecEnv, "an ArmKinematicPopulationVecEnv", PointCurriculumPopulation
    fused_env_type_ok = True
    # all env steps of a rollout in one launch per span (PPO's rollout_run_covered predicate on pop_env / pop_curriculum; KP1_ROLLOUT_RUN)
    _whole_rollout = PPO._whole_rollout


class RoutePopulationPPO(OneHandlePopulationPPO):
    """K route-curriculum runs of one PPOConfig on ONE RoutePopulationVecEnv (route_env.py): block k of its K N envs is replica k, which is the
    rollout buffers' replica-major layout, so every env step is one route step and one tracker launch (RoutePrefixCurriculumPopulation)
    whatever K is.  Everything else -- noise, truncation bootstrap, the epoch body, graph capture -- is PopulationPPO's.
    ``teacher_anchor``: a ``PopulationTeacherAnchor`` (teacher_anchor.py); the caller runs ``anchor.on_rollout_end(pop)`` between
    ``collect_rollouts()`` and ``train()``, as train_route does.

    Replica k is bit-identical to ``PPO(RouteVecEnv(..., seed=s_k), curriculum=RoutePrefixCurriculumDevice)`` on the same config
    (tests/test_route_population_gpu.py).  ``load_init_checkpoint`` (OneHandlePopulationPPO's) starts every replica from one checkpoint as
    train_route does.  The caller owns (and closes) the env and the tracker."""

    env_class, env_words, tracker_class = RoutePopulationVecEnv, "a RoutePopulationVecEnv", RoutePrefixCurriculumPopulation
    tracker_checks_k = False
    accepts_anchor = True
    fused_route_env_type_ok = True


class DockPopulationPPO(OneHandlePopulationPPO):
    """K Finisher (dock-mode) runs of one PPOConfig on ONE ArmKinematicPopulationVecEnv with ONE DockReverseCurriculumPopulation
    (finisher_tools.py): a promotion rewrites only its replica's live stage record, which the dock population forms of the step and reset
    kernels read per env, so replicas on different reverse-curriculum stages share a launch (and a wave).  Without a tracker the env is the
    plain dock step over K N envs.  Replica k is bit-identical to ``PPO(ArmKinematicVecEnv(..., seed=s_k), curriculum=DockReverseCurriculum)``
    on the same config (tests/test_dock_population_gpu.py).  ``load_init_checkpoint`` / ``load_init_checkpoints`` start the replicas from one
    checkpoint or one each (train_dock --seeds --resume-from).  The caller owns (and closes) the env and the tracker."""

    env_class, env_words, tracker_class = ArmKinematicPopulationVecEnv, "a dock-mode ArmKinematicPopulationVecEnv", DockReverseCurriculumPopulation
    env_also = staticmethod(lambda env: env.config.mode_name == "dock")
    fused_env_type_ok = True


def resolve_resume_population(resume_from: str | None, seeds: list[int], names: list[str] | None = None) -> list[str] | None:
    """train_dock / train --seeds --resume-from X, resolved on the host: None when X is not given or does not exist (a --seed run then starts
    from scratch too), [X] * K when X is a checkpoint zip (every seed starts from it), and X/<name_k>/model_latest.zip per replica when X is the
    root of an earlier --seeds run (``names``: the replica directories, seed_<s> by default).  Refuses a missing replica and, through
    check_init_checkpoints, checkpoints a population cannot resume together."""
    from pathlib import Path

    if not resume_from:
        return None
    root = Path(resume_from)
    if root.is_dir():
        names = names or [f"seed_{s}" for s in seeds]
        paths = [root / n / "model_latest.zip" for n in names]
        missing = [s for s, p in zip(seeds, paths) if not p.is_file()]
        if missing:
            raise ValueError(f"--resume-from {root}: no seed_<s>/model_latest.zip for seeds {missing} (a --seeds run root holds one per seed)")
        out = [str(p) for p in paths]
    elif root.exists():
        out = [str(root)] * len(seeds)
    else:
        return None
    OneHandlePopulationPPO.check_init_checkpoints(out)
    return out


# ---------------------------------------------------------------------------------------------------------------- trainer CLI (--seeds)
def parse_seeds(text: str) -> list[int]:
    """``--seeds 7,8,9,10`` -> [7, 8, 9, 10]"""
    try:
        seeds = [int(s) for s in str(text).split(",") if s.strip()]
    except ValueError as exc:
        raise ValueError(f"--seeds takes comma-separated integers, got {text!r}") from exc
    if not seeds:
        raise ValueError("--seeds needs at least one seed")
    return seeds


def parse_sweep(specs: list[str] | None) -> list[tuple[str, list[float]]]:
    """``--sweep KEY=v1,v2[,...]`` (repeatable) -> [(key, [v1, v2, ...]), ...] in the order given; refuses unknown and shape keys, a key
    given twice and values that are not finite numbers"""
    import math

    out: list[tuple[str, list[Any]]] = []
    for spec in specs or []:
        key, sep, values = str(spec).partition("=")
        key = key.strip()
        if not sep or not key:
            raise ValueError(f"--sweep takes KEY=v1,v2[,...], got {spec!r}")
        if key == "seed" or key in SHAPE_KEYS:
            raise ValueError(f"--sweep {key}: the replicas share the seed list and the rollout / minibatch geometry; sweepable: {', '.join(SWEEPABLE)}")
        if key not in SWEEPABLE:
            raise ValueError(f"--sweep: unknown key {key!r} (sweepable: {', '.join(SWEEPABLE)})")
        if any(k == key for k, _ in out):
            raise ValueError(f"--sweep {key} is given twice: list all its values in one --sweep {key}=v1,v2")
        none_ok = key == "target_kl"     # target_kl=0.01,0.03,none: a replica without the early stop
        try:
            vals = [None if none_ok and v.strip().lower() in NONE_WORDS else float(v) for v in values.split(",") if v.strip()]
        except ValueError as exc:
            raise ValueError(f"--sweep {key}: values must be numbers, got {values!r}") from exc
        if not vals or not all(v is None or math.isfinite(v) for v in vals):
            raise ValueError(f"--sweep {key}: needs at least one finite value, got {values!r}")
        out.append((key, vals))
    return out


def replica_name(seed: int, overrides: dict[str, float]) -> str:
    """the artifact directory of a replica: seed_<s> without overrides, else seed_<s>_<key>_<repr(value)> per override in order
    (seed_7_learning_rate_0.0001)"""
    return "_".join([f"seed_{int(seed)}"] + [f"{k}_{'none' if v is None else repr(float(v))}" for k, v in overrides.items()])


def plan_replicas(seeds_text: str | None, sweep_specs: list[str] | None) -> tuple[list[int], list[dict[str, float]] | None, list[str]]:
    """the trainers' ``--seeds`` [+ ``--sweep``] on the host: (replica seeds, per-replica overrides or None without --sweep, replica
    directory names).  Replicas are the Cartesian product seeds x sweep values, seed-major, at most MAX_REPLICAS; refused before any device
    work."""
    import itertools

    if sweep_specs and seeds_text is None:
        raise ValueError("--sweep needs --seeds: a sweep trains its settings together as one population")
    seeds = parse_seeds(seeds_text)
    sweep = parse_sweep(sweep_specs)
    if not sweep:
        check_overrides(seeds, None)
        return seeds, None, [replica_name(s, {}) for s in seeds]
    combos = [dict(zip([k for k, _ in sweep], vals)) for vals in itertools.product(*[v for _, v in sweep])]
    rep_seeds = [s for s in seeds for _ in combos]
    overrides = [dict(c) for _ in seeds for c in combos]
    if len(rep_seeds) > MAX_REPLICAS:
        raise ValueError(f"--seeds x --sweep makes {len(rep_seeds)} replicas; a population trains at most {MAX_REPLICAS}")
    overrides = check_overrides(rep_seeds, overrides)
    return rep_seeds, overrides, [replica_name(s, o) for s, o in zip(rep_seeds, overrides)]


def population_status(pop: PopulationPPO, it: int, steps: int, elapsed: float, *, tag: str = "population") -> str:
    """a population trainer's line at the logging cadence (ppo.run_training's ``status``; ``steps``: each replica's env steps of this run)"""
    stages = [c.read().stage_index if c is not None else -1 for c in pop.curricula]
    return f"[{tag}] it={it} steps/replica={pop.num_timesteps} aggregate fps={pop.K * steps / elapsed:,.0f} stages={stages}"


def population_summary(pop: PopulationPPO, rows: list[dict[str, Any]], *, wall_seconds: float, selection: str) -> dict[str, Any]:
    """population_summary.json: one row per replica (its directory name and overrides, final curriculum stage, last update stats, model
    paths, best score when a selection ran), the seed and overrides with the best score, the wall time and the aggregate env-steps/s of all
    replicas"""
    for k, r in enumerate(rows):
        r.setdefault("replica", replica_name(pop.seeds[k], pop.overrides[k]))
        r.setdefault("overrides", dict(pop.overrides[k]))
    scored = [r for r in rows if r.get("best_score") is not None]
    best = max(scored, key=lambda r: r["best_score"]) if scored else None
    return {"seeds": list(pop.seeds), "replicas": pop.K, "selection": selection,
            "best_seed": best["seed"] if best else None, "best_overrides": best["overrides"] if best else None,
            "best_replica": best["replica"] if best else None, "best_score": best["best_score"] if best else None,
            "per_seed": rows, "num_timesteps_per_seed": int(pop.num_timesteps), "wall_seconds": wall_seconds,
            "aggregate_env_steps_per_second": pop.K * pop.num_timesteps / max(wall_seconds, 1e-9)}
