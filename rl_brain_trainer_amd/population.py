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

``replica(k)`` is a view with what ``checkpoint.save`` and the evaluators read, so a replica saves as an ordinary single-policy archive.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
import time
from typing import Any, Callable

import numpy as np
import torch

from . import native
from .ppo import ACT_DIM, OBS_DIM, ActorCritic, Dist, PPO, PPOConfig

MAX_REPLICAS = 16     # KP1_MLP_MAX_REPLICAS


def _bind_policy(policy: ActorCritic, flat: torch.Tensor) -> None:
    """make `policy` a view on row `flat` of the population's [K, P] parameter buffer (values copied in first)"""
    flat.copy_(policy.flat)
    policy.flat = flat
    off = 0
    for name, shape in policy.spec:
        n = math.prod(shape)
        policy.views[name] = flat[off:off + n].view(shape)
        off += n


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
        self.obs_w = pop.obs_w
        self.dist = _ReplicaDist()
        self.actor_extra_steps = 0
        self.backend = "hip"
        self.device = pop.device

    adam_t = property(lambda self: self._pop.adam_t)
    num_timesteps = property(lambda self: self._pop.num_timesteps)
    n_train_calls = property(lambda self: self._pop.n_train_calls)
    last_stats = property(lambda self: self._pop.replica_stats(self.k))

    @torch.no_grad()
    def predict(self, obs: torch.Tensor, deterministic: bool = True) -> torch.Tensor:
        """model.predict(obs, deterministic=True): mean action clipped to the action space"""
        if not deterministic:
            raise NotImplementedError("a population replica predicts deterministically (evaluators use deterministic=True)")
        return self._pop.infer_policy(self.k).predict(obs)


class PopulationPPO:
    """K = len(seeds) PPO runs of one PPOConfig, trained together.  ``env_factory(seed)`` builds replica k's env handle (first env id 0);
    ``curriculum_factory(seed)`` (optional) its PointCurriculum / DockReverseCurriculum, attached to that handle."""

    def __init__(self, seeds: list[int], cfg: PPOConfig, env_factory: Callable[[int], Any], *,
                 curriculum_factory: Callable[[int], Any] | None = None, dist: Dist | None = None, use_graphs: bool = True,
                 teacher_anchor: Any = None) -> None:
        seeds = [int(s) for s in seeds]
        if not seeds:
            raise ValueError("PopulationPPO needs at least one seed")
        if len(seeds) > MAX_REPLICAS:
            raise ValueError(f"PopulationPPO trains at most {MAX_REPLICAS} replicas at once (got {len(seeds)} seeds)")
        if len(set(seeds)) != len(seeds):
            raise ValueError(f"PopulationPPO seeds must be distinct (got {seeds}): equal seeds train identical replicas")
        if cfg.hidden not in (64, 128):
            raise ValueError(f"PopulationPPO runs the layer-wise kernels of the 2x64 / 2x128 nets; hidden={cfg.hidden} is not supported "
                             "(the 2x256 tile kernels have no replica axis)")
        if teacher_anchor is not None:
            raise ValueError("PopulationPPO does not support the teacher-anchor side loss (per-replica actor step counts)")
        dist = dist or Dist()
        if dist.enabled:
            raise ValueError("PopulationPPO is single-process: data parallel (a torch.distributed process group) is not supported")
        self.seeds = seeds
        self.K = K = len(seeds)
        self.cfg = cfg
        self.cfgs = [dataclasses.replace(cfg, seed=s) for s in seeds]
        self.dist = dist
        self.L = native.load()
        self.envs: list[Any] = []
        self.curricula: list[Any] = []
        try:
            for s in seeds:
                env = env_factory(s)
                self.envs.append(env)
                if int(getattr(env, "obs_dim", OBS_DIM)) != OBS_DIM:
                    raise ValueError("PopulationPPO takes the 56-float ArmKinematicEnv observation; route envs (obs_dim 80) are not supported")
                if env.dtype != torch.float32:
                    raise ValueError("PopulationPPO drives the production f32 env")
            if len({e.n_envs for e in self.envs}) != 1:
                raise ValueError("every replica's env must have the same number of envs")
        except BaseException:
            for e in self.envs:
                e.close()
            raise
        env0 = self.envs[0]
        self.device = env0.device
        self.n_envs = N = env0.n_envs
        self.obs_dim = OBS_DIM
        self.obs_w = 64
        for s, env in zip(seeds, self.envs):
            cur = curriculum_factory(s) if curriculum_factory is not None else None
            if cur is not None:
                cur.attach(env)
            self.curricula.append(cur)
            env.set_obs_stride(self.obs_w)
        T, dev, KN = cfg.n_steps, self.device, K * N
        self.T = T
        # parameters / Adam moments / gradient: [K, P], replica k = what PPO(seed = s_k) holds
        self.policies = [ActorCritic(cfg.hidden, dev, seed=s, obs_dim=OBS_DIM) for s in seeds]
        P = self.policies[0].numel
        self.flat = torch.zeros((K, P), dtype=torch.float32, device=dev)
        for k, pol in enumerate(self.policies):
            _bind_policy(pol, self.flat[k])
        self.adam_m = torch.zeros_like(self.flat)
        self.adam_v = torch.zeros_like(self.flat)
        self.grad = torch.zeros_like(self.flat)
        self.stats_dev = torch.zeros((K, 4), dtype=torch.float32, device=dev)
        self.adam_t = 0
        self.n_train_calls = 0
        self.num_timesteps = 0       # per replica (what each replica's single run would count)
        # rollout buffers [T(+1), K N, ...]: replica k's envs are columns [k N, (k + 1) N)
        self.obs_buf = torch.zeros((T + 1, KN, self.obs_w), dtype=torch.float32, device=dev)
        self.term_obs_buf = torch.zeros((T, KN, self.obs_w), dtype=torch.float32, device=dev)
        self.act_buf = torch.zeros((T, KN, ACT_DIM), dtype=torch.float32, device=dev)
        self.clip_act = torch.zeros((KN, ACT_DIM), dtype=torch.float32, device=dev)
        self.logp_buf = torch.zeros((T, KN), dtype=torch.float32, device=dev)
        self.val_buf = torch.zeros((T, KN), dtype=torch.float32, device=dev)
        self.rew_buf = torch.zeros((T, KN), dtype=torch.float32, device=dev)
        self.done_buf = torch.zeros((T, KN), dtype=torch.uint8, device=dev)
        self.adv_buf = torch.zeros((T, KN), dtype=torch.float32, device=dev)
        self.ret_buf = torch.zeros((T, KN), dtype=torch.float32, device=dev)
        # the generators a single PPO(seed = s_k) owns (rank 0)
        self.gens = [torch.Generator(device=dev).manual_seed(s) for s in seeds]
        self._perm_rngs = [np.random.Generator(np.random.PCG64(np.random.SeedSequence([s, 0, 0x6B7031]))) for s in seeds]
        self.noise_rep = torch.zeros((K, T, N, ACT_DIM), dtype=torch.float32, device=dev)   # replica k's draw, as PPO.noise_all
        self.noise_all = torch.zeros((T, KN, ACT_DIM), dtype=torch.float32, device=dev)
        total = T * N
        self.perm = torch.zeros((K, total), dtype=torch.int64, device=dev)                   # replica-local shuffles
        # minibatch i of replica k = local positions [start_i, end_i) of its shuffle; the kernels read minibatch i as ONE [K][n_i] index
        # block at K * start_i of the gathered index vector
        bs = max(cfg.batch_size, 1)
        self._mb = [(s0, min(s0 + bs, total)) for s0 in range(0, total, bs)]
        src = [k * total + torch.arange(s0, e0) for s0, e0 in self._mb for k in range(K)]
        self._mb_src = torch.cat(src).to(dev)
        self._rep_off = (torch.arange(K, device=dev, dtype=torch.int64) * N).view(K, 1)
        max_steps = max(int(env0.config.c.termination.max_episode_steps), 1)
        self._trunc_cap = min(N * (T // max_steps + 1), T * N)
        from . import mlp as _mlp

        self._mlp = _mlp.MlpKernels(cfg.hidden, dev, max_batch=max(N, bs, self._trunc_cap), obs_dim=OBS_DIM, replicas=K)
        self._mlp.pack(self.flat)
        self.use_graphs = bool(use_graphs)
        self._rollout_graph = None
        self._rollout_graph_key = None
        self._epoch_graph = None
        self._epoch_graph_key = None
        self._epoch_warm = False
        self._kernels_warm = False
        self._needs_reset = True
        self._last_stats_dev: tuple[torch.Tensor, int] | None = None
        self._last_stats_host: list[dict[str, float]] = [{} for _ in range(K)]
        self._infer: dict[int, Any] = {}
        self.rollout_s = 0.0
        self.update_s = 0.0

    # ------------------------------------------------------------------ views
    def replica(self, k: int) -> ReplicaView:
        return ReplicaView(self, k)

    def close(self) -> None:
        for e in self.envs:
            e.close()
        self._mlp.close()

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

    def _sl(self, k: int) -> slice:
        return slice(k * self.n_envs, (k + 1) * self.n_envs)

    # ------------------------------------------------------------------ rollout
    def _draw_perm(self, k: int) -> None:
        total, out = self.T * self.n_envs, self.perm[k]
        if total < PPO.PERM_CIPHER_MIN:
            torch.randperm(total, device=self.device, generator=self.gens[k], out=out)
            return
        keys = self._perm_rngs[k].integers(0, 1 << 32, size=8, dtype=np.uint64).astype(np.uint32)
        native.check(self.L.kp1_random_permutation(self.device.index or 0, total, keys.ctypes.data_as(C.c_void_p), C.c_void_p(out.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _policy_env_step(self, t: int) -> None:
        self._mlp.forward(self.obs_buf[t], noise=self.noise_all[t], value=self.val_buf[t], action=self.act_buf[t], clipped=self.clip_act,
                          log_prob=self.logp_buf[t])
        for k, env in enumerate(self.envs):
            sl = self._sl(k)
            env.step_into(self.clip_act[sl], self.obs_buf[t + 1, sl], self.rew_buf[t, sl], self.done_buf[t, sl], self.term_obs_buf[t, sl], True)

    def _rollout_step(self, t: int) -> None:
        self._policy_env_step(t)
        for k, cur in enumerate(self.curricula):
            if cur is not None:
                cur.observe(self.done_buf[t, self._sl(k)], self.n_envs)

    def _bootstrap_truncated(self) -> None:
        """PPO._bootstrap_truncated per replica: the critic of replica k on its (at most cap) truncated terminal observations"""
        K, T, N, cap = self.K, self.T, self.n_envs, self._trunc_cap
        trunc = ((self.done_buf.view(T, K, N).permute(1, 0, 2) & 3) == 2).reshape(K, T * N)
        loc = torch.stack([torch.nonzero_static(trunc[k], size=cap, fill_value=0).view(-1) for k in range(K)])
        gidx = (loc // N) * (K * N) + self._rep_off + loc % N
        valid = torch.arange(cap, device=self.device).view(1, cap) < trunc.sum(dim=1, keepdim=True)
        sel = self.term_obs_buf.view(T * K * N, self.obs_w).index_select(0, gidx.view(-1))
        tv = torch.empty(K * cap, dtype=torch.float32, device=self.device)
        # one forward of `cap` rows per replica: the handle's max_batch is sized to hold them (max(N, batch, _trunc_cap) in __init__), so
        # unlike PPO nothing is chunked here -- shrinking max_batch below _trunc_cap would make this call fail
        self._mlp.forward(sel, value=tv)
        self.rew_buf.view(-1).index_add_(0, gidx.view(-1), torch.where(valid.view(-1), self.cfg.gamma * tv, torch.zeros_like(tv)))

    def _post_rollout(self) -> None:
        cfg = self.cfg
        KN = self.K * self.n_envs
        self._bootstrap_truncated()
        last_v = torch.empty(KN, dtype=torch.float32, device=self.device)
        self._mlp.forward(self.obs_buf[self.T], value=last_v)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        native.check(self.L.kp1_gae_scan(self.device.index or 0, C.c_void_p(self.rew_buf.data_ptr()), C.c_void_p(self.val_buf.data_ptr()),
                                         C.c_void_p(self.done_buf.data_ptr()), C.c_void_p(last_v.data_ptr()), cfg.gamma, cfg.gae_lambda,
                                         C.c_void_p(self.adv_buf.data_ptr()), C.c_void_p(self.ret_buf.data_ptr()), self.T, KN, C.c_void_p(stream)))

    def _envs_use_current_stream(self) -> None:
        for env in self.envs:
            env.use_current_stream()

    def _capture_rollout(self) -> None:
        """PPO._capture_rollout for K envs: a warm-up step between a device snapshot of every env and its restore, then ONE graph on one
        stream (no forked branches)"""
        if not self._kernels_warm:
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):
                for env in self.envs:
                    env.use_current_stream()
                    env.snapshot()
                self._policy_env_step(0)
                for k, cur in enumerate(self.curricula):
                    if cur is not None:
                        cur.observe(self.done_buf[0, self._sl(k)].zero_(), 0)
                self._post_rollout()
                for env in self.envs:
                    env.use_current_stream()
                    env.restore()
            torch.cuda.current_stream(self.device).wait_stream(side)
            self._kernels_warm = True
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._envs_use_current_stream()
            for t in range(self.T):
                self._rollout_step(t)
            self._post_rollout()
        self._rollout_graph = g
        self._envs_use_current_stream()

    @torch.no_grad()
    def collect_rollouts(self) -> None:
        T = self.T
        t0 = time.perf_counter()
        if self._needs_reset:
            for k, env in enumerate(self.envs):
                self.obs_buf[0, self._sl(k)].copy_(env.reset())
            self._needs_reset = False
        else:
            self.obs_buf[0].copy_(self.obs_buf[T])
        for k in range(self.K):
            self.noise_rep[k].normal_(generator=self.gens[k])
        self.noise_all.view(T, self.K, self.n_envs, ACT_DIM).copy_(self.noise_rep.permute(1, 0, 2, 3))
        if self.use_graphs:
            key = (tuple(getattr(e, "launch_args_version", 0) for e in self.envs), self.cfg.gamma, self.cfg.gae_lambda)
            if self._rollout_graph is None or self._rollout_graph_key != key:
                self._capture_rollout()
                self._rollout_graph_key = key
            self._rollout_graph.replay()
        else:
            for t in range(T):
                self._rollout_step(t)
            self._kernels_warm = True
            self._post_rollout()
        self.num_timesteps += T * self.n_envs
        self.rollout_s += time.perf_counter() - t0

    # ------------------------------------------------------------------ update
    def _epoch_key(self) -> tuple:
        c = self.cfg
        return (c.learning_rate, c.clip_range, c.ent_coef, c.vf_coef, c.max_grad_norm, c.adam_eps, c.batch_size, c.n_steps, c.normalize_advantage)

    def _epoch_body(self) -> None:
        """one update epoch from the shuffles in self.perm: global row indices, per-replica minibatch advantage statistics, then per minibatch
        loss_grad + Adam of all replicas"""
        cfg, K, N = self.cfg, self.K, self.n_envs
        total = self.T * N
        obs = self.obs_buf[:self.T].view(-1, self.obs_w)
        act = self.act_buf.view(-1, ACT_DIM)
        old_logp, adv, ret = self.logp_buf.view(-1), self.adv_buf.view(-1), self.ret_buf.view(-1)
        gperm = (self.perm // N) * (K * N) + self._rep_off + self.perm % N          # [K, T N] global rows
        mb_idx = gperm.view(-1).index_select(0, self._mb_src)
        stats = None
        if cfg.normalize_advantage:
            n_mb = len(self._mb)
            sums = torch.empty((K, n_mb, 3), dtype=torch.float64, device=self.device)
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            dev = self.device.index or 0
            for k in range(K):
                native.check(self.L.kp1_adv_minibatch_sums(dev, C.c_void_p(adv.data_ptr()), C.c_void_p(gperm[k].data_ptr()), total, cfg.batch_size,
                                                           C.c_void_p(sums[k].data_ptr()), stream))
            st = torch.empty((K, n_mb, 2), dtype=torch.float32, device=self.device)
            native.check(self.L.kp1_adv_minibatch_stats(dev, C.c_void_p(sums.data_ptr()), K * n_mb, C.c_void_p(st.data_ptr()), stream))
            stats = st.permute(1, 0, 2).contiguous()                                  # [n_mb][K][2]
        for i, (s0, e0) in enumerate(self._mb):
            n = e0 - s0
            idx = mb_idx[K * s0:K * e0]
            self._mlp.loss_grad(obs, idx, n, act, old_logp, adv, ret, clip_range=cfg.clip_range, ent_coef=cfg.ent_coef, vf_coef=cfg.vf_coef,
                                inv_count=1.0 / n, grad_out=self.grad, stats_out=self.stats_dev, adv_stats=None if stats is None else stats[i],
                                normalize=cfg.normalize_advantage)
            self._mlp.adam_step(self.flat, self.grad, self.adam_m, self.adam_v, lr=cfg.learning_rate, eps=cfg.adam_eps,
                                max_grad_norm=cfg.max_grad_norm, step=0, fused_norm=True)

    def train(self) -> None:
        cfg = self.cfg
        t0 = time.perf_counter()
        n_mb = len(self._mb)
        n_updates = 0
        self.n_train_calls += 1
        self.stats_dev.zero_()
        for _epoch in range(cfg.n_epochs):
            for k in range(self.K):
                self._draw_perm(k)
            if self.use_graphs:
                if self._epoch_graph is not None and self._epoch_graph_key != self._epoch_key():
                    self._epoch_graph = None
                if self._epoch_graph is None and not self._epoch_warm:
                    self._epoch_warm = True        # one eager epoch first (warm-up; a real epoch), as PPO
                    self._epoch_body()
                elif self._epoch_graph is None:
                    torch.cuda.synchronize(self.device)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._epoch_body()
                    self._epoch_graph, self._epoch_graph_key = g, self._epoch_key()
                    g.replay()
                else:
                    self._epoch_graph.replay()
            else:
                self._mlp.set_step_count(self.adam_t)
                self._epoch_body()
            n_updates += n_mb
            self.adam_t += n_mb
        self._last_stats_dev = (self.stats_dev.clone(), n_updates)
        self.update_s += time.perf_counter() - t0

    def replica_stats(self, k: int) -> dict[str, float]:
        """PPO.last_stats of replica k (reading it synchronises with the last update)"""
        if self._last_stats_dev is not None:
            stats, n_updates = self._last_stats_dev
            rows = (stats / max(n_updates, 1)).tolist()
            self._last_stats_host = [dict(zip(("policy_loss", "value_loss", "entropy", "approx_kl"), r), n_updates=n_updates) for r in rows]
            self._last_stats_dev = None
        return self._last_stats_host[k]

    def learn(self, total_timesteps: int | None = None, log_every: int = 0) -> "PopulationPPO":
        """PPO.learn for every replica: ``total_timesteps`` counts each replica's own env steps"""
        total = int(total_timesteps if total_timesteps is not None else self.cfg.total_timesteps)
        start = self.num_timesteps
        it, t0 = 0, time.time()
        while self.num_timesteps - start < total:
            self.collect_rollouts()
            self.train()
            it += 1
            if log_every and it % log_every == 0:
                dt = time.time() - t0
                print(f"[population] it={it} steps/replica={self.num_timesteps} aggregate fps={self.K * (self.num_timesteps - start) / dt:,.0f}", flush=True)
        return self


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


def learn_population(pop: PopulationPPO, total_timesteps: int, *, on_iteration=None, log_every: int = 0, tag: str = "population") -> float:
    """The trainers' loop for a population: iterations until every replica has taken `total_timesteps` env steps; ``on_iteration(pop)``
    after each (per-replica gates).  Returns the wall time in seconds."""
    t0 = time.time()
    start, it = pop.num_timesteps, 0
    while pop.num_timesteps - start < total_timesteps:
        pop.collect_rollouts()
        pop.train()
        it += 1
        if on_iteration is not None:
            on_iteration(pop)
        if log_every and it % log_every == 0:
            stages = [c.read().stage_index if c is not None else -1 for c in pop.curricula]
            print(f"[{tag}] it={it} steps/replica={pop.num_timesteps} aggregate fps={pop.K * (pop.num_timesteps - start) / (time.time() - t0):,.0f} "
                  f"stages={stages}", flush=True)
    torch.cuda.synchronize(pop.device)
    return time.time() - t0


def population_summary(pop: PopulationPPO, rows: list[dict[str, Any]], *, wall_seconds: float, selection: str) -> dict[str, Any]:
    """population_summary.json: one row per seed (final curriculum stage, last update stats, model paths, best score when a selection ran),
    the seed with the best score, the wall time and the aggregate env-steps/s of all replicas"""
    scored = [r for r in rows if r.get("best_score") is not None]
    best = max(scored, key=lambda r: r["best_score"]) if scored else None
    return {"seeds": list(pop.seeds), "replicas": pop.K, "selection": selection,
            "best_seed": best["seed"] if best else None, "best_score": best["best_score"] if best else None,
            "per_seed": rows, "num_timesteps_per_seed": int(pop.num_timesteps), "wall_seconds": wall_seconds,
            "aggregate_env_steps_per_second": pop.K * pop.num_timesteps / max(wall_seconds, 1e-9)}
