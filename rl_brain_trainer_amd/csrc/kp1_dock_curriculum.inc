// kp1_dock_curriculum.inc -- the Finisher's reverse curriculum as a device tracker (include/kp1_ppo.h, kp1_dock_curriculum_*).
// Included at the end of kp1_env.hip: it edits the env's live DevCfg<R> / DevSampler, which only that translation unit can name.
//
// Reference: DockReverseCurriculumCallback, kinematic_phase1/training/callbacks.py:104-212.  After every VecEnv step the callback walks the
// finished episodes in env order, keeps the last `window_episodes` success bits, and -- once the current stage has seen its minimum number of
// episodes and the last `stage window` of them pass the stage's threshold -- applies the next stage's overrides to every env
// (apply_dock_training_stage, arm_kinematic_env.py:459-487) and starts counting again.  Here the same rule is one wave on the rollout stream:
// each lane folds 64 done bytes into a done mask and a success mask, a ballot skips steps in which nothing ended, lane 0 replays the finished
// episodes in env order.  A promotion writes the next stage's (host-resolved, cumulative) values straight into the device config the step and
// reset kernels read, so the rollout needs no host callback and stays one hipGraph replay.
namespace {

// the values a stage can override, resolved on the host to what the env holds once stages 0..k have been applied in order
template <typename R>
__device__ __forceinline__ void dock_apply_stage(const kp1_dock_curriculum_stage& s, DevCfg<R>* __restrict__ cfg, DevSampler* __restrict__ smp) {
  cfg->env.action_delta_scale = (R)s.action_delta_scale;
  cfg->kin.action_delta_scale = s.action_delta_scale;   // the q-integration chain reads the fp64 copy (DevCfg::Kin)
  cfg->env.dock_residual_action_limit = (R)s.dock_residual_action_limit;
  cfg->env.dock_delta_q_change_limit_scale = (R)s.dock_delta_q_change_limit_scale;
  kp1_dock_reset& d = smp->dr;
  d.close_bucket_probability = s.close_bucket_probability;
  d.close_bucket_min_pos_error_m = s.close_bucket_min_pos_error_m;
  d.close_bucket_max_pos_error_m = s.close_bucket_max_pos_error_m;
  d.close_bucket_max_ori_error_rad = s.close_bucket_max_ori_error_rad;
  d.handoff_state_probability = s.handoff_state_probability;
  for (int k = 0; k < NJ; ++k) {
    d.close_init_q_noise[k] = s.close_init_q_noise[k];
    d.init_q_noise[k] = s.init_q_noise[k];
  }
  if (s.handoff_count >= 0) {   // this stage's slice of the (concatenated) handoff-state buffer
    smp->handoff_offset = s.handoff_offset;
    smp->n_handoff = s.handoff_count;
  }
}

// one block of n done bytes (KP1_DONE_* bits) in index order; lane 0 carries the tracker state.  apply(stage) is what a promotion does with the
// next stage's record: dock_apply_stage on the handle's config (single tracker), or a copy into the replica's live record (population).
template <typename Apply>
__device__ __forceinline__ void dock_curriculum_scan(kp1_dock_curriculum_state* __restrict__ st, const uint8_t* __restrict__ dones, int n, int clock_steps,
                                                     Apply apply) {
  const int lane = threadIdx.x;
  if (lane == 0) st->num_timesteps += clock_steps;
  for (int base = 0; base < n; base += 64 * 64) {
    unsigned long long ended = 0ull, won = 0ull;
    const int first = base + lane * 64;
    for (int b = 0; b < 64 && first + b < n; b += 8) {
      // 8 bytes at a time when the run is inside the buffer (rollout rows are 8-byte aligned for the env counts in use), else bytewise
      if (first + b + 8 <= n && ((uintptr_t)(dones + first + b) & 7) == 0) {
        const unsigned long long w = *reinterpret_cast<const unsigned long long*>(dones + first + b);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const unsigned int d = (unsigned int)(w >> (8 * k)) & 0xffu;
          if (d & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) {
            ended |= 1ull << (b + k);
            if (d & KP1_DONE_SUCCESS) won |= 1ull << (b + k);
          }
        }
      } else {
        for (int k = 0; k < 8 && first + b + k < n; ++k) {
          const unsigned int d = dones[first + b + k];
          if (d & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) {
            ended |= 1ull << (b + k);
            if (d & KP1_DONE_SUCCESS) won |= 1ull << (b + k);
          }
        }
      }
    }
    if (__ballot(ended != 0ull) == 0ull) continue;
    for (int src = 0; src < 64; ++src) {
      unsigned long long m = __shfl(ended, src);
      const unsigned long long w = __shfl(won, src);
      if (lane != 0) continue;
      const int cap = st->window_episodes;   // deque(maxlen = window_episodes)
      while (m) {
        const int bit = __ffsll((long long)m) - 1;
        m &= m - 1;
        st->stage_episode_count += 1;
        // ring: `ring_len` newest entries, the oldest at ring_head
        if (st->ring_len < cap) {
          st->ring[(st->ring_head + st->ring_len) % cap] = (uint8_t)((w >> bit) & 1ull);
          st->ring_len += 1;
        } else {
          st->ring[st->ring_head] = (uint8_t)((w >> bit) & 1ull);
          st->ring_head = (st->ring_head + 1) % cap;
        }
        const int k = st->stage_index;
        if (k >= st->n_stages - 1) continue;
        const kp1_dock_curriculum_stage& cur = st->stages[k];
        if (st->stage_episode_count < cur.min_episodes) continue;
        const int need = cur.window_episodes < cap ? cur.window_episodes : cap;
        if (st->ring_len < need) continue;
        const int take = cur.window_episodes < st->ring_len ? cur.window_episodes : st->ring_len;   // the newest `take` episodes
        int wins = 0;
        for (int j = 0; j < take; ++j) wins += st->ring[(st->ring_head + st->ring_len - 1 - j) % cap];
        const double rate = (double)wins / (double)take;
        if (rate < cur.success_rate_threshold) continue;
        apply(st->stages[k + 1]);
        if (st->n_events < KP1_DOCK_CURRICULUM_MAX_HISTORY) {
          kp1_dock_curriculum_event& ev = st->events[st->n_events];
          ev.from_stage = k;
          ev.to_stage = k + 1;
          ev.trigger_success_rate = rate;
          ev.stage_episode_count = st->stage_episode_count;
          ev.total_timesteps = st->num_timesteps;
        }
        st->n_events += 1;
        st->stage_index = k + 1;
        st->stage_episode_count = 0;
        st->ring_len = 0;
        st->ring_head = 0;
      }
    }
  }
}

// dones = [world][chunk_steps][n_local] (single process, one step: world = chunk_steps = 1): replayed step by step, rank by rank
template <typename R>
__global__ void __launch_bounds__(64) dock_curriculum_kernel(kp1_dock_curriculum_state* __restrict__ st, const uint8_t* __restrict__ dones, int n_local,
                                                             int chunk_steps, int world, int clock_steps, DevCfg<R>* __restrict__ cfg,
                                                             DevSampler* __restrict__ smp) {
  for (int t = 0; t < chunk_steps; ++t)
    for (int r = 0; r < world; ++r)
      dock_curriculum_scan(st, dones + ((int64_t)r * chunk_steps + t) * n_local, n_local, r == 0 ? clock_steps : 0,
                           [&](const kp1_dock_curriculum_stage& s) { dock_apply_stage<R>(s, cfg, smp); });
}

// K trackers in one launch (kp1_dock_curriculum_observe_population): workgroup k is dock_curriculum_kernel's rule on tracker k and the done
// bytes [k n, (k + 1) n) of its replica, its clock advancing by n as a single tracker's does.  A promotion writes only replica k: its tracker
// and its live stage record live[k], which the dock population forms of the step and reset kernels read.  The shared config is not touched.
__global__ void __launch_bounds__(64) dock_curriculum_population_kernel(kp1_dock_curriculum_state* __restrict__ states, kp1_dock_curriculum_stage* __restrict__ live,
                                                                        const uint8_t* __restrict__ dones_all, int n) {
  const int k = blockIdx.x;
  kp1_dock_curriculum_stage* __restrict__ rec = live + k;
  dock_curriculum_scan(states + k, dones_all + (int64_t)k * n, n, n, [&](const kp1_dock_curriculum_stage& s) { *rec = s; });
}

template <typename R>
__global__ void __launch_bounds__(64) dock_curriculum_apply_kernel(const kp1_dock_curriculum_state* __restrict__ st, DevCfg<R>* cfg, DevSampler* smp) {
  if (threadIdx.x == 0) dock_apply_stage<R>(st->stages[st->stage_index], cfg, smp);
}

// upload_cfg (kp1_update_config, kp1_set_handoff_states) rewrites the device config and sampler from the host mirror, i.e. with the BASE
// scalars and the whole handoff buffer: while a tracker is attached its current stage (scalars + handoff slice) is applied again on top.
// the stage tracker `st` stands at -> the handle's device config and sampler (one wave, lane 0 writes)
int apply_dock_stage(kp1_env* env, const kp1_dock_curriculum_state* st) {
  return with_real(env->real_type, [&](auto real) {
    using R = decltype(real);
    return launch_env(dock_curriculum_apply_kernel<R>, 64, 64, 0, env->stream, st, (DevCfg<R>*)env->dev_cfg, env->dev_smp);
  });
}
int reapply_dock_stage(kp1_env* env) { return env->dock_tracker ? apply_dock_stage(env, env->dock_tracker) : (int)KP1_OK; }

}  // namespace

extern "C" {

int kp1_dock_curriculum_create(kp1_env* env, const kp1_dock_curriculum_stage* stages_host, int32_t n_stages, int32_t window_episodes,
                               kp1_dock_curriculum_state** out_dev) {
  if (!env || !stages_host || !out_dev) return fail(KP1_ERR_INVALID, "NULL argument to kp1_dock_curriculum_create");
  if (env->mode != KP1_MODE_DOCK) return fail(KP1_ERR_INVALID, "the dock reverse curriculum drives a dock-mode env");
  if (env->pop_dock_states) return fail(KP1_ERR_UNSUPPORTED, "the handle is bound to a dock population: its stages are per replica");
  if (n_stages < 1 || n_stages > KP1_DOCK_CURRICULUM_MAX_STAGES) return fail(KP1_ERR_INVALID, "DockReverseCurriculumCallback requires 1..16 stages");
  const int window = window_episodes < 1 ? 1 : window_episodes;   // callbacks.py:116 max(..., 1)
  if (window > KP1_DOCK_CURRICULUM_MAX_WINDOW) return fail(KP1_ERR_INVALID, "window_episodes exceeds KP1_DOCK_CURRICULUM_MAX_WINDOW");
  for (int k = 0; k < n_stages; ++k)
    if (stages_host[k].handoff_count >= 0 && (stages_host[k].handoff_offset < 0 || stages_host[k].handoff_offset + stages_host[k].handoff_count > env->n_handoff))
      return fail(KP1_ERR_INVALID, "a stage's handoff slice lies outside the buffer given to kp1_set_handoff_states");
  HIP_TRY(hipSetDevice(env->device));
  kp1_dock_curriculum_state* h = new kp1_dock_curriculum_state();
  std::memset(h, 0, sizeof *h);
  h->n_stages = n_stages;
  h->window_episodes = window;
  for (int k = 0; k < n_stages; ++k) {
    h->stages[k] = stages_host[k];
    if (h->stages[k].min_episodes < 1) h->stages[k].min_episodes = 1;          // :144 max(int(stage.get("min_episodes", window)), 1)
    if (h->stages[k].window_episodes < 1) h->stages[k].window_episodes = 1;    // :146
  }
  kp1_dock_curriculum_state* d = nullptr;
  hipError_t e = hipMalloc((void**)&d, sizeof *h);
  if (e == hipSuccess) e = hipMemcpy(d, h, sizeof *h, hipMemcpyHostToDevice);
  delete h;
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    return fail(kp1::status_of(e), std::string("kp1_dock_curriculum_create: ") + hipGetErrorString(e));
  }
  // _on_training_start: the first stage is applied before the first reset (callbacks.py:128-129)
  const int rc = apply_dock_stage(env, d);
  if (rc != KP1_OK) {
    (void)hipFree(d);
    return rc;
  }
  env->dock_tracker = d;
  *out_dev = d;
  return KP1_OK;
}

int kp1_dock_curriculum_create_population(kp1_env* env, const kp1_dock_curriculum_stage* stages_host, int32_t n_stages, int32_t window_episodes,
                                          int32_t n_replicas, kp1_dock_curriculum_state** out_dev) {
  if (!env || !stages_host || !out_dev) return fail(KP1_ERR_INVALID, "NULL argument to kp1_dock_curriculum_create_population");
  if (env->mode != KP1_MODE_DOCK || env->cfg.env.mode != KP1_MODE_DOCK)
    return fail(KP1_ERR_UNSUPPORTED, "kp1_dock_curriculum_create_population: the dock reverse curriculum drives a dock-mode env");
  if (env->real_type != KP1_REAL_F32) return fail(KP1_ERR_UNSUPPORTED, "kp1_dock_curriculum_create_population: a population env handle is f32");
  if (n_replicas < 1 || n_replicas > KP1_CURRICULUM_MAX_REPLICAS)
    return fail(KP1_ERR_INVALID, "kp1_dock_curriculum_create_population: n_replicas must be in [1, KP1_CURRICULUM_MAX_REPLICAS]");
  if (env->n % n_replicas != 0)
    return fail(KP1_ERR_INVALID, "kp1_dock_curriculum_create_population: the env count must be a multiple of the replica count");
  if (env->pop_states || env->pop_dock_states)
    return fail(KP1_ERR_UNSUPPORTED, "kp1_dock_curriculum_create_population: the handle is already bound to a population");
  if (env->dock_tracker)
    return fail(KP1_ERR_UNSUPPORTED, "kp1_dock_curriculum_create_population: the handle carries a single dock tracker (kp1_dock_curriculum_create)");
  if (n_stages < 1 || n_stages > KP1_DOCK_CURRICULUM_MAX_STAGES) return fail(KP1_ERR_INVALID, "DockReverseCurriculumCallback requires 1..16 stages");
  const int window = window_episodes < 1 ? 1 : window_episodes;
  if (window > KP1_DOCK_CURRICULUM_MAX_WINDOW) return fail(KP1_ERR_INVALID, "window_episodes exceeds KP1_DOCK_CURRICULUM_MAX_WINDOW");
  for (int k = 0; k < n_stages; ++k)
    if (stages_host[k].handoff_count >= 0 && (stages_host[k].handoff_offset < 0 || stages_host[k].handoff_offset + stages_host[k].handoff_count > env->n_handoff))
      return fail(KP1_ERR_INVALID, "a stage's handoff slice lies outside the buffer given to kp1_set_handoff_states");
  HIP_TRY(hipSetDevice(env->device));
  // K trackers set up as kp1_dock_curriculum_create sets up one, then the K live stage records (stage 0 to begin with)
  static_assert(sizeof(kp1_dock_curriculum_state) % alignof(kp1_dock_curriculum_stage) == 0, "live records follow the trackers");
  const size_t bytes = (sizeof(kp1_dock_curriculum_state) + sizeof(kp1_dock_curriculum_stage)) * (size_t)n_replicas;
  std::vector<unsigned char> h(bytes, 0);
  kp1_dock_curriculum_state* hs = reinterpret_cast<kp1_dock_curriculum_state*>(h.data());
  kp1_dock_curriculum_stage* hl = reinterpret_cast<kp1_dock_curriculum_stage*>(hs + n_replicas);
  for (int r = 0; r < n_replicas; ++r) {
    kp1_dock_curriculum_state& t = hs[r];
    t.n_stages = n_stages;
    t.window_episodes = window;
    for (int k = 0; k < n_stages; ++k) {
      t.stages[k] = stages_host[k];
      if (t.stages[k].min_episodes < 1) t.stages[k].min_episodes = 1;
      if (t.stages[k].window_episodes < 1) t.stages[k].window_episodes = 1;
    }
    hl[r] = t.stages[0];
  }
  kp1_dock_curriculum_state* d = nullptr;
  hipError_t e = hipMalloc((void**)&d, bytes);
  if (e == hipSuccess) e = hipMemcpy(d, h.data(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    return fail(kp1::status_of(e), std::string("kp1_dock_curriculum_create_population: ") + hipGetErrorString(e));
  }
  // _on_training_start of every replica: stage 0 into the shared config before the first reset, as kp1_dock_curriculum_create does (what no
  // stage overrides is read from there; the population forms read the rest from the live records)
  const int rc = apply_dock_stage(env, d);
  if (rc != KP1_OK) {
    (void)hipFree(d);
    return rc;
  }
  env->pop_dock_states = d;   // not env->dock_tracker: upload_cfg must not copy one replica's stage into the shared config
  env->pop_replicas = n_replicas;
  *out_dev = d;
  return KP1_OK;
}

int kp1_dock_curriculum_observe_population(kp1_env* env, kp1_dock_curriculum_state* states_dev, const uint8_t* dones, int32_t n_per_replica,
                                           int32_t n_replicas, void* stream) {
  if (!env || !states_dev || !dones || n_per_replica <= 0 || n_replicas < 1 || n_replicas > KP1_CURRICULUM_MAX_REPLICAS)
    return fail(KP1_ERR_INVALID, "bad argument to kp1_dock_curriculum_observe_population");
  HIP_TRY(hipSetDevice(env->device));
  return launch_env(dock_curriculum_population_kernel, 64 * n_replicas, 64, 0, (hipStream_t)stream, states_dev,
                    reinterpret_cast<kp1_dock_curriculum_stage*>(states_dev + n_replicas), dones, n_per_replica);   // one wave per tracker
}

int kp1_dock_curriculum_read_replica(kp1_env* env, const kp1_dock_curriculum_state* states_dev, int32_t n_replicas, int32_t k,
                                     kp1_dock_curriculum_state* out_host, void* stream) {
  if (!env || !states_dev || !out_host) return fail(KP1_ERR_INVALID, "NULL argument");
  if (k < 0 || k >= n_replicas) return fail(KP1_ERR_INVALID, "replica index out of range");
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipMemcpyAsync(out_host, states_dev + k, sizeof *out_host, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return KP1_OK;   // (the handle's shared host mirror stays as it is: the replicas' stages differ)
}

int kp1_dock_curriculum_destroy(kp1_env* env, kp1_dock_curriculum_state* st_dev) {
  if (!env) return fail(KP1_ERR_INVALID, "NULL env");
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipStreamSynchronize(env->stream));
  if (env->dock_tracker == st_dev) env->dock_tracker = nullptr;
  if (st_dev && env->pop_dock_states == st_dev) {   // a dock population: the handle steps in the ordinary dock form again
    env->pop_dock_states = nullptr;
    env->pop_replicas = 0;
  }
  HIP_TRY(hipFree(st_dev));
  return KP1_OK;
}

int kp1_dock_curriculum_observe(kp1_env* env, kp1_dock_curriculum_state* st_dev, const uint8_t* dones, int32_t n_local, int32_t chunk_steps, int32_t world,
                                void* stream) {
  if (!env || !st_dev || !dones || n_local <= 0 || chunk_steps <= 0 || world <= 0) return fail(KP1_ERR_INVALID, "bad argument to kp1_dock_curriculum_observe");
  HIP_TRY(hipSetDevice(env->device));
  const int clock = n_local * world;
  return with_real(env->real_type, [&](auto real) {
    using R = decltype(real);
    return launch_env(dock_curriculum_kernel<R>, 64, 64, 0, (hipStream_t)stream, st_dev, dones, n_local, chunk_steps, world, clock, (DevCfg<R>*)env->dev_cfg,
                      env->dev_smp);
  });
}

int kp1_dock_curriculum_read(kp1_env* env, const kp1_dock_curriculum_state* st_dev, kp1_dock_curriculum_state* out_host, void* stream) {
  if (!env || !st_dev || !out_host) return fail(KP1_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipMemcpyAsync(out_host, st_dev, sizeof *out_host, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  // keep the host mirror of the config in step with what the device tracker applied (kp1_update_config re-uploads env->cfg)
  const kp1_dock_curriculum_stage& s = out_host->stages[out_host->stage_index];
  env->cfg.env.action_delta_scale = s.action_delta_scale;
  env->cfg.env.dock_residual_action_limit = s.dock_residual_action_limit;
  env->cfg.env.dock_delta_q_change_limit_scale = s.dock_delta_q_change_limit_scale;
  kp1_dock_reset& d = env->cfg.dock_reset;
  d.close_bucket_probability = s.close_bucket_probability;
  d.close_bucket_min_pos_error_m = s.close_bucket_min_pos_error_m;
  d.close_bucket_max_pos_error_m = s.close_bucket_max_pos_error_m;
  d.close_bucket_max_ori_error_rad = s.close_bucket_max_ori_error_rad;
  d.handoff_state_probability = s.handoff_state_probability;
  for (int k = 0; k < NJ; ++k) {
    d.close_init_q_noise[k] = s.close_init_q_noise[k];
    d.init_q_noise[k] = s.init_q_noise[k];
  }
  return KP1_OK;
}

}  // extern "C"
