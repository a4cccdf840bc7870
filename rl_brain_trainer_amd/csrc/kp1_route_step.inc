// kp1_route_step.inc -- device code of one route step: the wrapper-level reset sampler and reset, the route observation, the nearest-waypoint
// scan of one 8-lane group and route_step_lane, the step of one env (its statements: kp1_route_step_body.inc, shared with kp1_route_step_kernel).
// Included inside an anonymous namespace by kp1_route.inc (kp1_env.hip: kp1_route_reset_kernel / kp1_route_nearest_kernel / kp1_route_step_kernel)
// and by kp1_mlp.hip, whose route rollout kernel runs the policy forward of a row tile and the whole route step of the tile's envs in one launch
// (kp1_route_rollout_step.inc).  Needs kp1_device.hpp, kp1_env_step.inc (reset_env, the PCG64 stream helpers), include/kp1_route.h and
// include/kp1_ziggurat_tables.h.

__device__ const uint64_t ZIG_KI[256] = KP1_ZIGGURAT_KI;
__device__ const double ZIG_WI[256] = KP1_ZIGGURAT_WI;
__device__ const double ZIG_FI[256] = KP1_ZIGGURAT_FI;

// numpy random_standard_normal (256-layer ziggurat): one 64-bit word per draw in 98.5 % of the cases (numpy, 300,000 draws); the
// wedge, the tail (2.3e-4 per draw) and a repeated tail loop (1.3e-5) are forced on purpose by tests/test_forced_rng_*.py
__device__ __forceinline__ double pcg_standard_normal(Pcg& g) {
  for (;;) {
    uint64_t r = pcg_next64(g);
    const int idx = (int)(r & 0xff);
    r >>= 8;
    const int sign = (int)(r & 0x1);
    const uint64_t rabs = (r >> 1) & 0x000fffffffffffffULL;
    double x = (double)rabs * ZIG_WI[idx];
    if (sign) x = -x;
    if (rabs < ZIG_KI[idx]) return x;
    if (idx == 0) {
      for (;;) {
        const double xx = -KP1_ZIGGURAT_NOR_INV_R * log1p(-pcg_double(g));
        const double yy = -log1p(-pcg_double(g));
        if (yy + yy > xx * xx) return ((rabs >> 8) & 0x1) ? -(KP1_ZIGGURAT_NOR_R + xx) : KP1_ZIGGURAT_NOR_R + xx;
      }
    } else {
      if (((ZIG_FI[idx - 1] - ZIG_FI[idx]) * pcg_double(g) + ZIG_FI[idx]) < exp(-0.5 * x * x)) return x;
    }
  }
}
__device__ __forceinline__ double normal_scaled(Pcg& g, double std) {
#pragma clang fp contract(off)
  const double z = pcg_standard_normal(g);
  const double prod = std * z;   // loc + scale * z with loc = 0.0, product rounded before the add like numpy
  return 0.0 + prod;
}

struct RouteTable {  // device, fp64
  const double* q;        // [W][7]
  const double* pose;     // [W][6]
  const double* next_dq;  // [W][7]
  const double* progress; // [W]
  int n;
};

template <typename R>
struct RouteState {
  int32_t *cur, *start, *last, *streak, *completed, *reset_mode;
  uint8_t *ready, *wp_success, *regression, *ori_hit;
  R *q_error, *nearest;
  R* prev;          // SoA [27][N]: prev_q 7, prev_dq 7, prev_action 7, prev_pose 6
  uint64_t* rng64;  // [4][N]
  uint32_t* rng32;  // [2][N]
  double* scratch;  // [N][4*7] explicit-reset values for reset_env
  R* comps;         // [17][N] or nullptr
};
constexpr int RP_Q = 0, RP_DQ = 7, RP_ACT = 14, RP_POSE = 21, RP_NUM = 27;

struct RouteDevCfg {
  kp1_route_config c;   // (c.reset.min / max_route_index: the host's last set_window; the kernels read `window`)
  int success_dwell_steps, terminate_on_success;
  // reset window of each replica of a population handle: env i resets inside window[i / n_per_replica] (a single handle: n_per_replica = N,
  // window 0).  The prefix tracker of replica k rewrites window[k] on promotion.
  int n_per_replica, pad_;
  int32_t window[KP1_ROUTE_MAX_REPLICAS][2];   // [min_route_index, max_route_index]
};

// the reset window of env i
__device__ __forceinline__ void route_window_of(const RouteDevCfg& rc, int64_t i, int& lo, int& hi) {
  const int k = (int)i / rc.n_per_replica;
  lo = rc.window[k][0];
  hi = rc.window[k][1];
}

__device__ __forceinline__ int rclipi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// route_reset_samplers.py:47-117 on the wrapper's stream; all values fp64
struct RouteSampleDev {
  double initial_q[NJ], initial_dq[NJ], initial_prev_action[NJ];
  int route_index, start_index, mode;
};
// (win_min / win_max: the env's reset window, in place of c.min_route_index / c.max_route_index)
__device__ __forceinline__ void sample_route_reset_dev(Pcg& g, const RouteTable& rt, const DevSampler& smp, const kp1_route_reset_cfg& c, int win_min,
                                                       int win_max, RouteSampleDev& out) {
  const int max_index = rt.n - 1;
  const int lo = rclipi(win_min, 1, max_index);
  const int hi = rclipi(win_max, lo, max_index);
  double ratios[5] = {fmax(c.prefix_start_reset_ratio, 0.0), fmax(c.random_prefix_reset_ratio, 0.0), fmax(c.segment_reset_ratio, 0.0),
                      fmax(c.replay_reset_ratio, 0.0), fmax(c.recovery_reset_ratio, 0.0)};
  double total = 0.0;
#pragma unroll
  for (int i = 0; i < 5; ++i) total += ratios[i];
  if (total > 0.0) {
#pragma unroll
    for (int i = 0; i < 5; ++i) ratios[i] /= total;
  } else {
    ratios[0] = 0.0; ratios[1] = 1.0; ratios[2] = 0.0; ratios[3] = 0.0; ratios[4] = 0.0;
  }
  // Generator.choice(p=): cdf = cumsum(p) / cdf[-1]; searchsorted(cdf, random(), side="right")
  double cdf[5], acc = 0.0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    acc += ratios[i];
    cdf[i] = acc;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) cdf[i] /= acc;
  const double u = pcg_double(g);
  int mode = 0;  // searchsorted(side="right") = number of cdf entries <= u (cdf is non-decreasing)
#pragma unroll
  for (int i = 0; i < 5; ++i) mode += cdf[i] <= u ? 1 : 0;
  if (c.mode >= 1 && c.mode <= 5) mode = c.mode - 1;
  int route_index, start_index;
  if (mode == KP1_ROUTE_MODE_PREFIX_START) {
    route_index = pcg_integers(g, lo, hi + 1);
    start_index = 0;
  } else if (mode == KP1_ROUTE_MODE_SEGMENT) {
    const int seg_lo = rclipi(c.segment_start_index, 1, max_index);
    const int seg_hi = rclipi(c.segment_end_index, seg_lo, max_index);
    route_index = pcg_integers(g, seg_lo, (seg_hi < hi ? seg_hi : hi) + 1);
    start_index = route_index - 1 > 0 ? route_index - 1 : 0;
  } else if (mode == KP1_ROUTE_MODE_REPLAY) {
    const int rlo = rclipi(c.replay_start_index, 1, max_index);
    const int rhi = rclipi(c.replay_end_index, rlo, max_index);
    route_index = pcg_integers(g, rlo, (rhi < hi ? rhi : hi) + 1);
    start_index = route_index - 1 > 0 ? route_index - 1 : 0;
  } else {
    route_index = pcg_integers(g, lo, hi + 1);
    start_index = route_index - 1 > 0 ? route_index - 1 : 0;
  }
  const int src = rclipi(mode == KP1_ROUTE_MODE_RECOVERY ? route_index : start_index, 0, max_index);
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    const double noise = c.q_noise_std > 0.0 ? normal_scaled(g, c.q_noise_std) : 0.0;
    out.initial_q[k] = dclip(rt.q[src * NJ + k] + noise, smp.lower[k], smp.upper[k]);
  }
#pragma unroll
  for (int k = 0; k < NJ; ++k) out.initial_dq[k] = c.dq_noise_std > 0.0 ? normal_scaled(g, c.dq_noise_std) : 0.0;
#pragma unroll
  for (int k = 0; k < NJ; ++k) out.initial_prev_action[k] = dclip(c.prev_action_noise_std > 0.0 ? normal_scaled(g, c.prev_action_noise_std) : 0.0, -1.0, 1.0);
  out.route_index = route_index;
  out.start_index = start_index;
  out.mode = mode;
}

// 56 base floats -> the wrapper's observation row (route_observation.py:31-61 in the key-sorted flat layout)
template <typename R>
__device__ __forceinline__ void store_route_obs(float* __restrict__ obs, int64_t i, int obs_dim, int obs_stride, const float* o, const DevCfg<R>& cfg, const RouteTable& rt,
                                                int cur, const R* q) {
  float* dst = obs + i * obs_stride;   // row pitch >= obs_dim (the padding of the PPO buffers is never written and stays zero)
  if (obs_dim == KP1_OBS_DIM) {
#pragma unroll
    for (int k = 0; k < KP1_OBS_DIM; ++k) dst[k] = o[k];
    return;
  }
#pragma unroll
  for (int k = 0; k < 47; ++k) dst[k] = o[k];
  const int w = rclipi(cur, 0, rt.n - 1), wt = rclipi(cur - 1 > 0 ? cur - 1 : 0, 0, rt.n - 1);
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    const R goal = (R)rt.q[w * NJ + k], tangent = (R)rt.next_dq[wt * NJ + k];
    const R span = kp_max<R>(cfg.upper[k] - cfg.lower[k], (R)1e-9), dl = kp_max<R>(cfg.dlim[k], (R)1e-9);
    dst[47 + k] = (float)kp_clip<R>((goal - q[k]) / dl, (R)-1, (R)1);                                  // route_q_error
    dst[54 + k] = (float)kp_clip<R>((R)2 * ((goal - cfg.lower[k]) / span) - (R)1, (R)-1, (R)1);         // route_q_goal
    dst[64 + k] = (float)kp_clip<R>(tangent / dl, (R)-1, (R)1);                                         // route_tangent
  }
  const int max_route_index = rt.n - 1;
  const R s0 = (R)cur / (R)(max_route_index > 1 ? max_route_index : 1);
  const R s1 = (R)rt.progress[w] / kp_max<R>((R)rt.progress[rt.n - 1], (R)1e-9);
  dst[61] = (float)kp_clip<R>(s0, (R)0, (R)1);
  dst[62] = (float)kp_clip<R>(s1, (R)0, (R)1);
  dst[63] = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) dst[71 + k] = o[47 + k];
}

// shared tail of reset and auto-reset: base reset with explicit state, wrapper bookkeeping, observation
template <typename R>
__device__ __forceinline__ void route_reset_env(const EnvState<R>& st, const DevCfg<R>& cfg, const DevSampler& smp, const RouteDevCfg& rc, const RouteTable& rt,
                                                const RouteState<R>& rs, int64_t i, int first_target, int start_index, int mode, const double* q0,
                                                const double* dq0, const double* pa0, float* obs, int obs_dim, int obs_stride, int win_max) {
  const int64_t n = st.n;
  int cur = first_target, last = first_target;
  if (rc.c.sequence_enabled) {
    const int max_index = win_max < rt.n - 1 ? win_max : rt.n - 1;
    const int seq_len = rc.c.sequence_length > 1 ? rc.c.sequence_length : 1;
    cur = rclipi(first_target, 1, max_index);
    last = max_index < cur + seq_len - 1 ? max_index : cur + seq_len - 1;
  }
  // explicit-state arrays for reset_env, four [N][7] planes (it indexes them with i * 7 + k)
  double* s_q = rs.scratch, *s_dq = rs.scratch + NJ * n, *s_pa = rs.scratch + 2 * NJ * n, *s_goal = rs.scratch + 3 * NJ * n;
  const int w = rclipi(cur, 0, rt.n - 1);
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    s_q[i * NJ + k] = q0[k];
    s_dq[i * NJ + k] = dq0[k];
    s_pa[i * NJ + k] = pa0[k];
    s_goal[i * NJ + k] = rt.q[w * NJ + k];
  }
  ResetOptsDev o;
  o.initial_q = s_q; o.initial_dq = s_dq; o.initial_prev_action = s_pa; o.goal_q = s_goal;
  o.goal_pose6 = nullptr;
  o.flags = OPT_INITIAL_Q | OPT_INITIAL_DQ | OPT_INITIAL_PREV_ACTION | OPT_GOAL_Q;
  float ob[KP1_OBS_DIM];
  reset_env<R, KP1_MODE_APPROACH>(st, cfg, smp, nullptr, o, 0, i, ob);
  rs.cur[i] = cur; rs.start[i] = start_index; rs.last[i] = last; rs.streak[i] = 0; rs.completed[i] = 0; rs.reset_mode[i] = mode;
  R q[NJ];
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    q[k] = st.r(F_Q + k, i);
    rs.prev[(RP_Q + k) * n + i] = q[k];
    rs.prev[(RP_DQ + k) * n + i] = st.r(F_DQ + k, i);
    rs.prev[(RP_ACT + k) * n + i] = st.r(F_PREV_ACTION + k, i);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) rs.prev[(RP_POSE + k) * n + i] = st.r(F_EE_POSE + k, i);
  if (obs) store_route_obs<R>(obs, i, obs_dim, obs_stride, ob, cfg, rt, cur, q);
}

template <typename R>
struct RouteStepArgs {
  EnvState<R> st; const DevCfg<R>* cfg; const DevSampler* smp; const RouteDevCfg* rc; RouteTable rt; RouteState<R> rs;
  const R* actions; const uint8_t* base_done; float* obs; R* reward; uint8_t* done; float* terminal_obs; int obs_dim, obs_stride, auto_reset;
};

// Nearest waypoint in joint space, min over the whole route of ||Q_w - q|| (route_env.py: nearest_route_q_distance), for one group of 8 lanes
// that share an env: lane `sub` takes the waypoints sub, sub + 8, ... of the table `route_q` ([W][7] in LDS, in the env's real type), three
// xor-shuffles combine the partial minima; every lane of the group returns sqrt(min) (sqrt is monotone: taken once).  Whole groups must call it.
template <typename R>
__device__ __forceinline__ R route_nearest_group(const R* __restrict__ route_q, int W, int sub, const R* q) {
  R best = std::numeric_limits<R>::infinity();
  for (int wv = sub; wv < W; wv += 8) {
    R s = (R)0;
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
      const R d = route_q[wv * NJ + k] - q[k];
      s += d * d;
    }
    best = s < best ? s : best;
  }
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) {
    const R o = __shfl_xor(best, off);
    best = o < best ? o : best;
  }
  return kp_sqrt(best);
}

// route_env.py:124-192 / route_sequence_env.py:150-236 for env i, after the base step has advanced the base env and rs.nearest[i] is written
// (kp1_route_step_kernel's statements after kp1_route_step_kernel's declarations: the same text, see kp1_route_step_body.inc)
template <typename R>
__device__ __forceinline__ void route_step_lane(const RouteStepArgs<R>& a, int64_t i) {
  const double* __restrict__ route_q = a.rt.q;   // [W][7] fp64; the two rows a step needs are cast to the env's real type on load
  const int W = a.rt.n;
  const int64_t n = a.st.n;
#include "kp1_route_step_body.inc"
}

// ---- chained sequential evaluation (kp1_route_chain_*): what kp1_route_chain_kernel (kp1_route.inc) and the one-launch chain step of kp1_mlp.hip
// (kp1_route_chain_step.inc) share
struct RouteChainDev {   // device arrays [R] unless noted
  const int32_t *start, *end;
  int32_t *wp, *steps, *first_ready, *max_streak, *n_records;
  uint8_t* alive;
  float *min_pos, *min_ori, *min_q;
  kp1_route_chain_record* records;   // [R][max_len]
  int32_t* n_alive;                  // [1]
  int max_len, stop_on_failure;
};

template <typename R>
struct RouteChainArgs {
  EnvState<R> st; const DevCfg<R>* cfg; const DevSampler* smp; const RouteDevCfg* rc; RouteTable rt; RouteState<R> rs;
  RouteChainDev ch; const uint8_t* done; float* obs; int32_t* tags; int obs_dim, obs_stride;
};

// the bookkeeping of a fresh episode: the minima of position and orientation error start from the planes reset_env wrote, and the record
// keeps q as the reset left it (the evaluator's initial joint-space error is taken from it on the host)
template <typename R>
__device__ __forceinline__ void route_chain_open(const EnvState<R>& st, const RouteChainDev& ch, int64_t i, int waypoint) {
  ch.wp[i] = waypoint; ch.steps[i] = 0; ch.first_ready[i] = -1; ch.max_streak[i] = 0;
  ch.min_pos[i] = (float)st.r(F_POS_ERR, i);
  ch.min_ori[i] = (float)st.r(F_ORI_ERR, i);
  ch.min_q[i] = std::numeric_limits<float>::infinity();
  const int slot = waypoint - ch.start[i];
  if (slot >= 0 && slot < ch.max_len) {
#pragma unroll
    for (int k = 0; k < NJ; ++k) ch.records[i * ch.max_len + slot].start_q[k] = st.q_load(k, i);
  }
}

// one chain step of row i after its route step (kp1_route_chain_kernel's statements after kp1_route_chain_kernel's declarations: the same text,
// see kp1_route_chain_body.inc); returns whether the row is still running
template <typename R>
__device__ __forceinline__ int route_chain_lane(const RouteChainArgs<R>& a, int64_t i) {
  const EnvState<R>& st = a.st;
  const RouteChainDev& ch = a.ch;
  int alive_after = 0;
  {
#include "kp1_route_chain_body.inc"
  }
  return alive_after;
}
