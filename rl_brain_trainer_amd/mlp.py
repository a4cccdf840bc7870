"""Python handle on the MFMA actor-critic kernels (include/kp1_ppo.h, csrc/kp1_mlp.hip)."""
from __future__ import annotations

import ctypes as C

import torch

from . import native

OBS_DIM, OBS_PAD, ACT_DIM = 56, 64, 7


_p = native.ptr


def span_split(first_step: int, n_steps: int, cap: int) -> list[tuple[int, int]]:
    """[first_step, first_step + n_steps) as consecutive (start, count) spans of at most ``cap`` steps"""
    if n_steps < 1 or cap < 1:
        raise ValueError("span_split needs n_steps >= 1 and cap >= 1")
    return [(t0, min(cap, first_step + n_steps - t0)) for t0 in range(first_step, first_step + n_steps, cap)]


class MlpKernels:
    def __init__(self, hidden: int, device: torch.device, max_batch: int = 8192, obs_dim: int = OBS_DIM, replicas: int = 1) -> None:
        """replicas > 1: a population handle (kp1_mlp_create_population) -- K independent nets trained through one launch sequence; every
        per-net buffer gains a leading replica axis (include/kp1_ppo.h documents the layouts)."""
        self.L = native.load()
        L = self.L
        self.hidden = hidden
        self.device = device
        self.max_batch = int(max_batch)
        self._h = C.c_void_p()
        self.obs_dim = int(obs_dim)                      # 56, or 80 with the route observation keys
        self.obs_pad = 64 if self.obs_dim <= 64 else 128   # row pitch the kernels also accept (zero padded)
        self.fused = True                                # what set_fused last set (hidden 256: the tile kernels; the handle's default is on)
        self.train_tile = False                          # what set_train_tile last set (hidden 64 / 128: train_tile128_kernel; default off)
        self.kl_gate = False                             # whether set_kl_gate has a gate set (default: none)
        self.hparam_line = False                         # whether the kernels read the handle's hyper-parameter table (hparams_store / set_replica_hparams)
        if replicas == 1:
            native.check(L.kp1_mlp_create_ex(native.device_index(device), hidden, self.obs_dim, self.max_batch, C.byref(self._h)))
        else:
            native.check(L.kp1_mlp_create_population(native.device_index(device), hidden, self.obs_dim, self.max_batch, int(replicas), C.byref(self._h)))
        self.replicas = int(L.kp1_mlp_replicas(self._h))
        self.num_params = int(L.kp1_mlp_num_params_ex(hidden, self.obs_dim))

    def close(self) -> None:
        if self._h.value:
            self.L.kp1_mlp_destroy(self._h)
            self._h = C.c_void_p()

    OPT_FUSED = native.header_int("KP1_MLP_OPT_FUSED")

    def set_fused(self, on: bool) -> None:
        """hidden = 256: whole activation chain of a 32-row tile in one workgroup (default) vs the layer-wise kernels."""
        native.check(self.L.kp1_mlp_set_option(self._h, self.OPT_FUSED, int(bool(on))))
        self.fused = bool(on)

    OPT_ACTOR_EXTRA_STEPS = native.header_int("KP1_MLP_OPT_ACTOR_EXTRA_STEPS")

    def set_actor_extra_steps(self, steps: int) -> None:
        """Adam steps the actor tensors have taken beyond the common count (teacher-anchor side updates, teacher_anchor.py)."""
        native.check(self.L.kp1_mlp_set_option(self._h, self.OPT_ACTOR_EXTRA_STEPS, int(steps)))

    OPT_STEP_COUNT = native.header_int("KP1_MLP_OPT_STEP_COUNT")

    def set_step_count(self, steps: int) -> None:
        """Device-resident optimiser step count (restoring a checkpoint's Adam state)."""
        native.check(self.L.kp1_mlp_set_option(self._h, self.OPT_STEP_COUNT, int(steps)))

    OPT_BF16X3_WGRAD = native.header_int("KP1_MLP_OPT_BF16X3_WGRAD")

    def set_bf16x3_wgrad(self, on: bool) -> None:
        """EXPERIMENT (default off): weight-gradient GEMMs on operands pre-split into three bf16 pieces, six bf16 MFMAs per product block
        (gemm_tn_bf16x3_kernel).  Not the exact path; bench.py's value never uses it."""
        native.check(self.L.kp1_mlp_set_option(self._h, self.OPT_BF16X3_WGRAD, int(bool(on))))

    OPT_TRAIN_TILE = native.header_int("KP1_MLP_OPT_TRAIN_TILE")

    def set_train_tile(self, on: bool) -> None:
        """hidden 64 / 128 (default off): loss_grad of a minibatch of at most 2048 rows per replica runs forward, loss and backward of a 32-row
        tile of one net in ONE launch (train_tile128_kernel) in place of the five layer-wise launches; larger minibatches keep those.
        hidden 256 refuses (its tile path is ``set_fused``)."""
        native.check(self.L.kp1_mlp_set_option(self._h, self.OPT_TRAIN_TILE, int(bool(on))))
        self.train_tile = bool(on)

    OPT_PROFILE = native.header_int("KP1_MLP_OPT_PROFILE")
    PROFILE_SLOTS = ("mlp_train_tile", "gemm_tn_split", "grad_finalize", "adam")

    def set_profile(self, on: bool) -> None:
        """HIP-event pairs around every launch of the optimiser step (eager launches only); read with ``profile_read``."""
        native.check(self.L.kp1_mlp_set_option(self._h, self.OPT_PROFILE, int(bool(on))))

    def profile_read(self) -> dict[str, dict[str, float]]:
        """average in-situ duration (us) and launch count of each optimiser-step kernel since the last read"""
        us = (C.c_float * 4)()
        cnt = (C.c_int32 * 4)()
        native.check(self.L.kp1_mlp_profile_read(self._h, C.cast(us, C.c_void_p), C.cast(cnt, C.c_void_p)))
        return {name: {"us": float(us[i]), "launches": int(cnt[i])} for i, name in enumerate(self.PROFILE_SLOTS)}

    HPARAM_FIELDS = ("learning_rate", "adam_eps", "max_grad_norm", "clip_range", "ent_coef", "vf_coef")   # kp1_replica_hparams

    def set_replica_hparams(self, rows: list[dict[str, float]] | None) -> None:
        """Population handles: per-replica PPO hyper-parameters (kp1_mlp_set_replica_hparams), one dict with every HPARAM_FIELDS key per
        replica; replica k's loss / Adam kernels then read row k in place of the scalar arguments.  None clears the table."""
        if rows is None:
            native.check(self.L.kp1_mlp_set_replica_hparams(self._h, None, 0, self._stream()))
            self.hparam_line = False
            return
        table = (C.c_float * (len(rows) * len(self.HPARAM_FIELDS)))(*[float(r[f]) for r in rows for f in self.HPARAM_FIELDS])
        native.check(self.L.kp1_mlp_set_replica_hparams(self._h, C.cast(table, C.c_void_p), len(rows), self._stream()))
        self.hparam_line = True

    def hparams_store(self, rows: list[dict[str, float]]) -> None:
        """Every handle, K = 1 included: the same table written by one small launch on the current stream (kp1_mlp_hparams_store) -- no copy
        from host memory, no wait; launches queued before it read the old values, later ones (and later replays of a captured graph, which
        holds only the table's address) the new.  One dict with every HPARAM_FIELDS key per replica, rounded to fp32 here as a scalar
        argument would be.  From the first call on the kernels read the table in place of loss_grad's and adam_step's scalars;
        ``set_replica_hparams(None)`` returns the handle to them."""
        table = (C.c_float * (len(rows) * len(self.HPARAM_FIELDS)))(*[float(r[f]) for r in rows for f in self.HPARAM_FIELDS])
        native.check(self.L.kp1_mlp_hparams_store(self._h, C.cast(table, C.c_void_p), len(rows), self._stream()))
        self.hparam_line = True

    def set_kl_gate(self, targets: list[float | None] | None) -> None:
        """SB3 PPO's ``target_kl`` as a device decision (kp1_mlp_set_kl_gate): one target per replica, None = that replica never stops.
        While a gate is set, a replica whose minibatch approx_kl exceeds 1.5 * target takes neither that minibatch's Adam step nor any
        later one until ``kl_gate_arm``, and adds nothing more to ``stats_out``; the Adam step count is kept per replica.  ``None`` (the
        argument) clears the gate, which is refused while the replicas' step counts differ."""
        if targets is None:
            native.check(self.L.kp1_mlp_set_kl_gate(self._h, None, 0, self._stream()))
            self.kl_gate = False
            return
        arr = (C.c_double * len(targets))(*[float("nan") if t is None else float(t) for t in targets])
        native.check(self.L.kp1_mlp_set_kl_gate(self._h, C.cast(arr, C.c_void_p), len(targets), self._stream()))
        self.kl_gate = True

    def kl_gate_arm(self) -> None:
        """a new train() call: every replica's record is cleared in one launch (kp1_mlp_kl_gate_arm; the thresholds stay)"""
        native.check(self.L.kp1_mlp_kl_gate_arm(self._h, self._stream()))

    def kl_gate_read(self, stream: torch.cuda.Stream | None = None) -> tuple[list[dict[str, float | int]], list[int]]:
        """(one record per replica -- threshold, stopped, n_counted, n_seen, stop_index, stop_kl --, the replicas' Adam step counts); waits
        for ``stream`` (default: the current one)"""
        rec = (native.KlGate * self.replicas)()
        steps = (C.c_int32 * self.replicas)()
        st = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        native.check(self.L.kp1_mlp_kl_gate_read(self._h, C.cast(rec, C.c_void_p), C.cast(steps, C.c_void_p), st))
        fields = [f for f, _ in native.KlGate._fields_ if f != "reserved0"]
        return [{f: getattr(r, f) for f in fields} for r in rec], [int(v) for v in steps]

    def _stream(self):
        return native.stream_arg(self.device)

    def pack(self, flat_params: torch.Tensor) -> None:
        assert flat_params.numel() == self.replicas * self.num_params and flat_params.dtype == torch.float32 and flat_params.is_contiguous()
        native.check(self.L.kp1_mlp_pack_weights(self._h, _p(flat_params), self._stream()))

    def forward(self, obs: torch.Tensor, *, noise=None, mean=None, value=None, action=None, clipped=None, log_prob=None) -> None:
        """obs [n, obs_dim | obs_pad] contiguous f32; outputs written in place (None = skip).  Population handles: obs holds K * n rows,
        replica-major, and so does every output."""
        assert obs.shape[0] % self.replicas == 0
        n, stride = obs.shape[0] // self.replicas, obs.shape[1]
        assert obs.is_contiguous() and obs.dtype == torch.float32
        native.check(self.L.kp1_mlp_forward(self._h, _p(obs), stride, n, _p(noise), _p(mean), _p(value), _p(action), _p(clipped), _p(log_prob), self._stream()))

    def forward_env_step(self, env, obs: torch.Tensor, *, noise, value, action, log_prob, next_obs, reward, done, terminal_obs) -> None:
        """One rollout step in one launch (kp1_mlp_forward_env_step): policy.forward on `obs` (row m = env m of `env`), sampling, and
        VecEnv.step of every env with auto-reset, written into the caller's rollout buffers.

        hidden 256: a K = 1 handle on the tile kernels and a plain fp32 ArmKinematicVecEnv.  hidden 64 / 128: a K = 1 or a population handle
        (replica k owns rows [k n, (k + 1) n) of every buffer, n = env.n_envs / K) and an fp32 ArmKinematicVecEnv or an
        ArmKinematicPopulationVecEnv of K replicas whose bound trackers give each replica its own stage; ``next_obs`` and ``terminal_obs`` must not overlap ``obs``.
        ``value``, ``log_prob`` and ``terminal_obs`` may be None.  Refused: the 80-float route observation and route envs (they have no
        kp1_env step of their own), f64 envs, recorded reward components, modes other than approach / dock, a replica-count mismatch."""
        from .vec_env import ArmKinematicVecEnv

        if not isinstance(env, ArmKinematicVecEnv):
            raise TypeError(f"forward_env_step steps an ArmKinematicVecEnv or an ArmKinematicPopulationVecEnv handle; {type(env).__name__} "
                            "(route envs wrap their base env in a route step of their own) takes forward + step_into")
        assert obs.is_contiguous() and obs.dtype == torch.float32 and obs.shape[0] == env.n_envs
        native.check(self.L.kp1_mlp_forward_env_step(self._h, env._handle, _p(obs), obs.shape[1], _p(noise), _p(value), _p(action), _p(log_prob),
                                                     _p(next_obs), _p(reward), _p(done), _p(terminal_obs), self._stream()))

    def rollout_run(self, env, obs_buf: torch.Tensor, *, noise, value, action, log_prob, reward, done, terminal_obs, first_step: int, n_steps: int,
                    trackers=None, steps_per_call: int = 0) -> None:
        """Env steps ``first_step .. first_step + n_steps - 1`` of a rollout in one launch per span (kp1_rollout_run), plus one wide launch
        for the critic when ``value`` is given: per step exactly what ``forward_env_step`` (and ``trackers.observe`` after it) does, bit for
        bit.  ``obs_buf`` [T + 1, K n, pitch] is the whole rollout buffer (slice t + 1 is step t's next_obs); ``noise`` / ``action``
        [T, K n, 7], ``value`` / ``log_prob`` / ``reward`` / ``done`` [T, K n] and ``terminal_obs`` [T, K n, pitch] likewise, all contiguous;
        ``value``, ``log_prob`` and ``terminal_obs`` may be None.  A span longer than ``native.ROLLOUT_RUN_MAX_STEPS`` is split into
        consecutive calls, which leave everything as one call would.

        Covered: hidden 64 / 128, a K = 1 or a population handle, an fp32 ArmKinematicVecEnv / ArmKinematicPopulationVecEnv in approach mode,
        the 56-float observation at pitch 56 or 64.  ``trackers``: the PointCurriculum (K = 1) or PointCurriculumPopulation attached to
        ``env``; the launch then also runs the tracker (every clock + ``steps_per_call`` per env step), which needs at most 32 envs per
        replica.  None: nothing observes, a bound env's stage stays where it is.  Refused: hidden 256, route envs and the 80-float
        observation, f64 envs, recorded reward components, the dock mode, a replica-count mismatch, trackers the env is not attached to."""
        from .vec_env import ArmKinematicVecEnv

        if not isinstance(env, ArmKinematicVecEnv):
            raise TypeError(f"rollout_run steps an ArmKinematicVecEnv or an ArmKinematicPopulationVecEnv handle; {type(env).__name__} "
                            "(route envs wrap their base env in a route step of their own) takes the per-step rollout")
        T = obs_buf.shape[0] - 1
        assert obs_buf.is_contiguous() and obs_buf.dtype == torch.float32 and obs_buf.dim() == 3 and obs_buf.shape[1] == env.n_envs
        assert 0 <= first_step and n_steps >= 1 and first_step + n_steps <= T
        for buf in (noise, value, action, log_prob, reward, done, terminal_obs):
            assert buf is None or (buf.is_contiguous() and buf.shape[0] >= first_step + n_steps and buf.shape[1] == env.n_envs)
        st = C.c_void_p(trackers.device_state) if trackers is not None else None
        for t0, cnt in span_split(first_step, n_steps, native.ROLLOUT_RUN_MAX_STEPS):
            sl = lambda buf: _p(buf[t0]) if buf is not None else None   # noqa: E731
            native.check(self.L.kp1_rollout_run(self._h, env._handle, sl(obs_buf), obs_buf.shape[2], sl(noise), sl(value), sl(action), sl(log_prob),
                                                sl(reward), sl(done), sl(terminal_obs), cnt, st, int(steps_per_call), self._stream()))

    def forward_route_step(self, env, obs: torch.Tensor, *, noise, value, action, log_prob, next_obs, reward, done, terminal_obs) -> None:
        """One rollout step of a route env in one launch (kp1_mlp_forward_route_step, include/kp1_route.h): ``forward`` on `obs` (row m = env
        m of `env`) with sampling, then ``env.step_into(clipped, next_obs, reward, done, terminal_obs, True)``, bit for bit.

        ``env``: a RouteVecEnv, or a RoutePopulationVecEnv of K replicas with a population handle of K (replica k owns rows [k n, (k + 1) n)
        of every buffer).  hidden 64 / 128; the handle's obs_dim is the env's (56 or 80) and ``obs``'s pitch the one set with
        ``env.set_obs_stride``; ``next_obs`` and ``terminal_obs`` must not overlap ``obs``.  ``value``, ``log_prob`` and ``terminal_obs`` may
        be None.  Refused: hidden 256, f64 envs, recorded reward components, routes longer than ROUTE_FUSED_MAX_WAYPOINTS, a live RouteChain,
        a replica-count, obs_dim or pitch mismatch."""
        from .route_env import RouteVecEnv

        if not isinstance(env, RouteVecEnv):
            raise TypeError(f"forward_route_step steps a RouteVecEnv or a RoutePopulationVecEnv handle; {type(env).__name__} takes "
                            "forward_env_step (arm envs) or forward + step_into")
        assert obs.is_contiguous() and obs.dtype == torch.float32 and obs.shape[0] == env.n_envs
        native.check(self.L.kp1_mlp_forward_route_step(self._h, env._handle, _p(obs), obs.shape[1], _p(noise), _p(value), _p(action), _p(log_prob),
                                                       _p(next_obs), _p(reward), _p(done), _p(terminal_obs), self._stream()))

    def mean_value(self, obs: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        n = obs.shape[0]
        mean = torch.empty((n, ACT_DIM), dtype=torch.float32, device=obs.device)
        value = torch.empty(n, dtype=torch.float32, device=obs.device)
        for s in range(0, n, self.max_batch):
            e = min(s + self.max_batch, n)
            self.forward(obs[s:e], mean=mean[s:e], value=value[s:e])
        return mean, value

    def loss_grad(self, obs: torch.Tensor, idx: torch.Tensor | None, n: int, actions, old_logp, adv, ret, *, clip_range: float, ent_coef: float,
                  vf_coef: float, inv_count: float, grad_out: torch.Tensor, stats_out: torch.Tensor | None, adv_stats: torch.Tensor | None = None,
                  normalize: bool = True) -> None:
        assert obs.is_contiguous() and grad_out.numel() == self.replicas * self.num_params
        assert self.replicas == 1 or (idx is not None and idx.numel() == self.replicas * n)
        inv_std = 0.0 if normalize else -1.0
        native.check(self.L.kp1_mlp_loss_grad(self._h, _p(obs), obs.shape[-1], _p(idx), n, _p(actions), _p(old_logp), _p(adv), _p(ret), 0.0, inv_std,
                                              _p(adv_stats), clip_range, ent_coef, vf_coef, inv_count, _p(grad_out), _p(stats_out), 0, self._stream()))

    def adam_step(self, params, grad, exp_avg, exp_avg_sq, *, lr: float, eps: float, max_grad_norm: float, step: int,
                  fused_norm: bool = False) -> None:
        """fused_norm: grad is exactly what the last loss_grad call wrote (no all-reduce in between), so the sum-of-squares
        partials its finalize kernel left are reused and the separate norm reduction launch is skipped."""
        native.check(self.L.kp1_mlp_adam_step(self._h, _p(params), _p(grad), _p(exp_avg), _p(exp_avg_sq), lr, eps, max_grad_norm, step,
                                              2 if fused_norm else 0, self._stream()))

    def anchor_loss_grad(self, obs: torch.Tensor, idx: torch.Tensor | None, n: int, teacher_actions: torch.Tensor, *, loss_weight: float,
                         grad_out: torch.Tensor, loss_out: torch.Tensor) -> None:
        """The teacher-anchor side loss (kp1_mlp_anchor_loss_grad): obs [M, obs_dim | obs_pad] and teacher_actions [M, 7] are the dataset, idx
        int64 [K, n] its rows per replica ([n] or None for K = 1).  grad_out [K, P] gets the gradient of the six actor tensors and zeros
        elsewhere, loss_out [K] the losses.  The device step count is not advanced."""
        assert obs.is_contiguous() and obs.dtype == torch.float32 and teacher_actions.is_contiguous() and teacher_actions.dtype == torch.float32
        assert teacher_actions.shape == (obs.shape[0], ACT_DIM) and grad_out.numel() == self.replicas * self.num_params
        assert loss_out.numel() == self.replicas and loss_out.dtype == torch.float32
        assert idx is None or (idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == self.replicas * n)
        native.check(self.L.kp1_mlp_anchor_loss_grad(self._h, _p(obs), obs.shape[-1], _p(idx), n, _p(teacher_actions), loss_weight, _p(grad_out),
                                                     _p(loss_out), self._stream()))

    def anchor_adam_step(self, params, grad, exp_avg, exp_avg_sq, *, lr: float, eps: float, max_grad_norm: float, step: int) -> None:
        """clip_grad_norm_ + Adam on the actor tensors for the gradient the last anchor_loss_grad wrote (kp1_mlp_anchor_adam_step); the
        handle's actor-extra step count is one larger afterwards."""
        native.check(self.L.kp1_mlp_anchor_adam_step(self._h, _p(params), _p(grad), _p(exp_avg), _p(exp_avg_sq), lr, eps, max_grad_norm, step,
                                                     self._stream()))

    def placement_check(self, n_rows: int) -> dict[str, int | float]:
        """where the hardware puts the workgroups of a training-tile launch for an n_rows minibatch (the two placement assumptions the update
        kernels' SPEED rests on: include/kp1_ppo.h kp1_mlp_placement_check)"""
        out = (C.c_int32 * 8)()
        native.check(self.L.kp1_mlp_placement_check(native.device_index(self.device), int(n_rows), C.cast(out, C.c_void_p), self._stream()))
        wgs, pairs, same, rr, cus, used, arrived, xcds = (int(v) for v in out)
        return {"workgroups": wgs, "compute_units": cus, "compute_units_used": used, "second_tile_on_same_cu": same, "second_tile_pairs": pairs,
                "on_xcd_of_block_index_mod_8": rr, "xcds_among_first_8_blocks": xcds, "all_resident": arrived == wgs}

    def time_kernels(self, obs: torch.Tensor, n: int, iters: int = 20) -> dict[str, dict[str, float]]:
        """HIP-event timings of the MFMA GEMM kernels at minibatch size n (bench.py roofline block)."""
        ms = (C.c_float * 6)()
        fl = (C.c_double * 6)()
        native.check(self.L.kp1_mlp_time_kernels(self._h, _p(obs), obs.shape[-1], n, iters, C.cast(ms, C.c_void_p), C.cast(fl, C.c_void_p), self._stream()))
        names = ("gemm_nt_fwd_l2", "gemm_nt_bwd_dz1", "gemm_tn_dw2", "gemm_nt_fwd_l1", "mlp_train_tile", "gemm_tn_split")
        return {nm: {"ms": float(ms[i]), "flops": float(fl[i]), "tflops": float(fl[i]) / (float(ms[i]) * 1e-3) / 1e12}
                for i, nm in enumerate(names) if ms[i] > 0}
