// kp1_route.inc -- route-curriculum environments on the device (include/kp1_route.h; SURVEY.md 8a / a15).
// Included at the end of kp1_env.hip: uses its EnvState / DevCfg / reset_env / launch_step and the PCG64 stream helpers.
//
// A route step = the base approach step kernel (reward discarded, no auto-reset), the nearest-waypoint scan over the whole route
// (kp1_route_nearest_kernel: 8 lanes per env, the table in LDS) and ONE route kernel that does everything else the Python wrappers
// do around base_env.step(): route-ready test and streak, the 13-term route reward, waypoint hand-over inside the episode (new goal, entry
// metrics re-captured, observation rebuilt), the 24 route observation floats, termination, and the wrapper-level
// auto-reset (route reset sampler on the wrapper's own PCG64 stream, then the base reset with explicit state).
#include "../../include/kp1_route.h"
#include "../../include/kp1_ziggurat_tables.h"

namespace {

#include "kp1_route_step.inc"

template <typename R>
struct RouteResetArgs {
  EnvState<R> st; const DevCfg<R>* cfg; const DevSampler* smp; const RouteDevCfg* rc; RouteTable rt; RouteState<R> rs;
  const uint8_t* mask; const int32_t* route_index; const int32_t* start_index; const double* initial_q; const double* initial_dq; const double* initial_pa;
  float* obs; int obs_dim, obs_stride, evaluator_state;
};

template <typename R>
__global__ void __launch_bounds__(256) kp1_route_reset_kernel(const RouteResetArgs<R> a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.st.n || (a.mask && !a.mask[i])) return;
  const RouteDevCfg& rc = *a.rc;
  int win_min, win_max;
  route_window_of(rc, i, win_min, win_max);
  double q0[NJ], dq0[NJ], pa0[NJ];
  int first_target, start, mode;
  if (a.route_index) {  // explicit (route_env.py:53-60 / route_sequence_env.py:103-109)
    first_target = a.route_index[i];
    start = a.start_index ? a.start_index[i] : (first_target - 1 > 0 ? first_target - 1 : 0);
    const bool seq = rc.c.sequence_enabled != 0 || a.evaluator_state != 0;
    const int ws = rclipi(start, 0, a.rt.n - 1);
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
      q0[k] = (seq && a.initial_q) ? a.initial_q[i * NJ + k] : a.rt.q[ws * NJ + k];
      dq0[k] = (seq && a.initial_dq) ? a.initial_dq[i * NJ + k] : 0.0;
      pa0[k] = (seq && a.initial_pa) ? a.initial_pa[i * NJ + k] : 0.0;
    }
    mode = KP1_ROUTE_MODE_EXPLICIT;
  } else {
    Pcg g;
    rng_load(a.rs.rng64, a.rs.rng32, a.st.n, i, g);
    RouteSampleDev s;
    sample_route_reset_dev(g, a.rt, *a.smp, rc.c.reset, win_min, win_max, s);
    rng_store(a.rs.rng64, a.rs.rng32, a.st.n, i, g);
    first_target = s.route_index; start = s.start_index; mode = s.mode;
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
      q0[k] = s.initial_q[k]; dq0[k] = s.initial_dq[k]; pa0[k] = s.initial_prev_action[k];
    }
  }
  route_reset_env<R>(a.st, *a.cfg, *a.smp, rc, a.rt, a.rs, i, first_target, start, mode, q0, dq0, pa0, a.obs, a.obs_dim, a.obs_stride, win_max);
}

// The nearest-waypoint scan (route_nearest_group) over all envs.  As a per-env serial scan inside the step kernel it was a 484-iteration latency
// chain on a handful of waves (the whole step 76 us at 2048 envs); here 8 lanes share an env and the route table sits in LDS in the env's real
// type.  Same per-waypoint arithmetic, min is order-free: bitwise identical.
constexpr size_t KP1_ROUTE_MAX_TABLE_LDS_BYTES = 128 * 1024;   // of the CU's 160 KB
template <typename R>
__global__ void __launch_bounds__(256) kp1_route_nearest_kernel(const EnvState<R> st, const RouteTable rt, R* __restrict__ nearest) {
  extern __shared__ double route_q_lds_raw[];
  R* route_q = reinterpret_cast<R*>(route_q_lds_raw);  // [W][7]
  const int W = rt.n;
  for (int e = threadIdx.x; e < W * NJ; e += blockDim.x) route_q[e] = (R)rt.q[e];
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = t >> 3, n = st.n;
  const int sub = (int)(t & 7);
  const int64_t ic = i < n ? i : n - 1;   // whole groups of 8 lanes stay in the shuffles
  R q[NJ];
#pragma unroll
  for (int k = 0; k < NJ; ++k) q[k] = st.r(F_Q + k, ic);
  const R d = route_nearest_group<R>(route_q, W, sub, q);
  if (sub == 0 && i < n) nearest[i] = d;
}

// route_env.py:124-192 / route_sequence_env.py:150-236, after the base step kernel has advanced the base env
template <typename R>
__global__ void __launch_bounds__(256) kp1_route_step_kernel(const RouteStepArgs<R> a) {
  const double* __restrict__ route_q = a.rt.q;   // [W][7] fp64; the two rows a step needs are cast to the env's real type on load
  const int W = a.rt.n;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = a.st.n;
  if (i >= n) return;
#include "kp1_route_step_body.inc"
}

}  // namespace

// ============================================================================================ host
#include "kp1_route_host.hpp"

namespace {

int route_upload_cfg(kp1_route* r) {
  RouteDevCfg d;
  d.c = r->cfg;
  d.success_dwell_steps = r->base->cfg.termination.success_dwell_steps;
  d.terminate_on_success = r->base->cfg.termination.terminate_on_success;
  d.n_per_replica = r->n_per_replica;
  d.pad_ = 0;
  std::memset(d.window, 0, sizeof d.window);
  for (int k = 0; k < r->n_replicas; ++k) {
    d.window[k][0] = r->win[2 * k];
    d.window[k][1] = r->win[2 * k + 1];
  }
  HIP_TRY(hipMemcpyAsync(r->dev_cfg, &d, sizeof d, hipMemcpyHostToDevice, r->base->stream));
  HIP_TRY(hipStreamSynchronize(r->base->stream));
  return KP1_OK;
}

// what RouteResetArgs<R>, RouteStepArgs<R> and RouteChainArgs<R> have in common: the base env's state and config, the route's, the caller's
// observation rows
template <typename R, typename Args>
void fill_route_args(Args& a, const kp1_route* r, float* obs) {
  const kp1_env* e = r->base;
  a.st = state_of<R>(e); a.cfg = (const DevCfg<R>*)e->dev_cfg; a.smp = e->dev_smp; a.rc = r->dev_cfg; a.rt = route_table_of(r); a.rs = route_state_of<R>(r);
  a.obs = obs; a.obs_dim = kp1_route_obs_dim(r); a.obs_stride = r->obs_stride;
}

template <typename R>
int route_launch_reset(kp1_route* r, const uint8_t* mask, const int32_t* ri, const int32_t* si, const double* q0, const double* dq0, const double* pa0,
                       int evaluator_state, float* obs) {
  RouteResetArgs<R> a;
  fill_route_args<R>(a, r, obs);
  a.mask = mask; a.route_index = ri; a.start_index = si; a.initial_q = q0; a.initial_dq = dq0; a.initial_pa = pa0; a.evaluator_state = evaluator_state;
  return launch_env(kp1_route_reset_kernel<R>, r->n, ENV_BLOCK, 0, r->base->stream, a);
}

template <typename R>
int route_launch_step(kp1_route* r, const void* actions, float* obs, void* reward, uint8_t* done, float* terminal_obs, int auto_reset) {
  kp1_env* e = r->base;
  const int64_t n = e->n;
  uint8_t* base_done = r->bytes + 4 * n;
  const int32_t saved_stride = e->obs_stride;
  e->obs_stride = KP1_OBS_DIM;
  int rc = launch_step<R>(e, actions, r->base_obs, r->base_reward, base_done, nullptr, 0);
  e->obs_stride = saved_stride;
  if (rc != KP1_OK) return rc;
  RouteStepArgs<R> a;
  fill_route_args<R>(a, r, obs);
  a.actions = (const R*)actions; a.base_done = base_done; a.reward = (R*)reward; a.done = done; a.terminal_obs = terminal_obs; a.auto_reset = auto_reset;
  // the joint table of the whole route lives in LDS in the env's real type (27 KB at W = 484 in fp64): above the 64 KB a launch gets by
  // default the limit has to be raised explicitly, and kp1_route_create refuses tables that cannot fit the CU's 160 KB at all
  const size_t lds = sizeof(R) * (size_t)r->n_waypoints * NJ;
  if (lds > KP1_ROUTE_MAX_TABLE_LDS_BYTES) return fail(KP1_ERR_INVALID, "route joint table exceeds the LDS budget of kp1_route_nearest_kernel");
  if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)kp1_route_nearest_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // 8 lanes per env; the 32 envs of a 256-lane workgroup share one LDS copy of the table
  rc = launch_env(kp1_route_nearest_kernel<R>, n * 8, 256, lds, e->stream, a.st, a.rt, a.rs.nearest);
  return rc != KP1_OK ? rc : launch_env(kp1_route_step_kernel<R>, n, ENV_BLOCK, 0, e->stream, a);
}

int route_seed_streams(kp1_route* r, uint64_t seed0, uint64_t first_env_id) {
  return seed_planes_by(r->rng64, r->rng32, r->n, r->base->stream, [=](int64_t i) { return seed0 + first_env_id + (uint64_t)i; });
}

}  // namespace

// ---------------------------------------------------------------------------------------------- prefix curriculum on the device
// RoutePrefixCurriculumCallback._on_step (route_curriculum.py:84-121).  One wave.  Each lane condenses 64 consecutive envs into a
// done mask and four flag masks; a ballot skips steps in which no episode ended; finished episodes are then replayed strictly in env
// order by lane 0 (the masks of lane k arrive by shuffle), which is what the reference's sequential scan over `dones` does.  The
// single-process tracker (route_curriculum_kernel) and the data-parallel chunk tracker (route_curriculum_chunk_kernel) differ only in
// where the masks come from; the replay below is theirs in common.
namespace {

// the tracker fields lane 0 keeps in registers while it replays
struct RouteTrk {
  int stage, count, len, head, window;
  int sums[4];
};

__device__ __forceinline__ void route_trk_load(const kp1_route_curriculum_state* st, RouteTrk& c) {
  c.stage = st->stage_index; c.count = st->stage_episode_count; c.len = st->ring_len; c.head = st->ring_head; c.window = st->window_episodes;
#pragma unroll
  for (int q = 0; q < 4; ++q) c.sums[q] = st->ring_sums[q];
}

__device__ __forceinline__ void route_trk_store(kp1_route_curriculum_state* st, const RouteTrk& c) {
  st->stage_index = c.stage; st->stage_episode_count = c.count; st->ring_len = c.len; st->ring_head = c.head;
#pragma unroll
  for (int q = 0; q < 4; ++q) st->ring_sums[q] = c.sums[q];
}

// one finished episode (success, route_ready, orientation hit, regression): the four deque appends, the window rates, the promotion with its
// event record and the reset-window write (`win`: the tracker's replica window in the device route config).  `now` = the callback's
// num_timesteps at this env step.
__device__ __forceinline__ void route_trk_append(kp1_route_curriculum_state* __restrict__ st, int32_t* __restrict__ win, RouteTrk& c,
                                                 const uint8_t v[4], int64_t now) {
  c.count += 1;
  const int slot = c.len < c.window ? (c.head + c.len) % c.window : c.head;   // deque(maxlen = window).append
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (c.len >= c.window) c.sums[q] -= st->ring[q][slot];                   // the evicted oldest entry
    st->ring[q][slot] = v[q];
    c.sums[q] += v[q];
  }
  if (c.len < c.window) c.len += 1;
  else c.head = (c.head + 1) % c.window;
  if (c.count < st->min_episodes_per_stage || c.len < c.window) return;
  double rate[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) rate[q] = (double)c.sums[q] / (double)c.len;
  if (!(rate[0] >= st->promotion_success_rate && rate[1] >= st->promotion_route_ready_hit_rate && rate[2] >= st->promotion_orientation_hit_rate &&
        rate[3] <= st->promotion_max_regression_rate))
    return;
  if (c.stage >= st->n_stages - 1) return;   // _promote returns without touching anything on the last stage
  if (st->n_events < KP1_ROUTE_CURRICULUM_MAX_HISTORY) {
    kp1_route_curriculum_event& ev = st->events[st->n_events];
    ev.total_timesteps = now;
    ev.from_stage = c.stage; ev.to_stage = c.stage + 1;
    ev.from_prefix_end_index = st->prefix_end_index[c.stage]; ev.to_prefix_end_index = st->prefix_end_index[c.stage + 1];
    ev.recent_success_rate = rate[0]; ev.recent_route_ready_hit_rate = rate[1]; ev.recent_orientation_hit_rate = rate[2];
    ev.recent_regression_rate = rate[3];
  }
  st->n_events += 1;
  c.stage += 1;
  c.count = 0; c.len = 0; c.head = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) c.sums[q] = 0;
  win[0] = 1;                                                  // env_method("set_route_window", max_route_index = prefix, min_route_index = 1)
  win[1] = st->prefix_end_index[c.stage];
}

// the masks of one 64-env group per lane: bit b = env (group start + b)
struct RouteMasks {
  unsigned long long done, succ, ready, ori, regr;
};

// lane 0 appends the finished episodes of the 64 groups of the wave in env order (lane k's masks arrive by shuffle)
__device__ __forceinline__ void route_trk_replay(kp1_route_curriculum_state* __restrict__ st, int32_t* __restrict__ win, RouteTrk& c, int lane,
                                                 const RouteMasks& mk, int64_t now) {
  for (int src = 0; src < 64; ++src) {
    unsigned long long m = __shfl(mk.done, src);
    const unsigned long long ms = __shfl(mk.succ, src), mr = __shfl(mk.ready, src), mo = __shfl(mk.ori, src), mg = __shfl(mk.regr, src);
    if (lane != 0) continue;
    while (m) {
      const int b = __ffsll((long long)m) - 1;
      m &= m - 1;
      const uint8_t v[4] = {(uint8_t)((ms >> b) & 1ull), (uint8_t)((mr >> b) & 1ull), (uint8_t)((mo >> b) & 1ull), (uint8_t)((mg >> b) & 1ull)};
      route_trk_append(st, win, c, v, now);
    }
  }
}

// Workgroup k = replica k (a single handle: one workgroup): tracker st[k], envs [k n, (k + 1) n), window k.
__global__ void __launch_bounds__(64) route_curriculum_kernel(kp1_route_curriculum_state* __restrict__ st_all, RouteDevCfg* __restrict__ cfg,
                                                              const uint8_t* __restrict__ dones_all, const uint8_t* __restrict__ ready_all,
                                                              const uint8_t* __restrict__ ori_hit_all, const uint8_t* __restrict__ regression_all, int n,
                                                              int steps_per_call) {
  const int lane = threadIdx.x;
  const int rep = (int)blockIdx.x;
  kp1_route_curriculum_state* __restrict__ st = st_all + rep;
  int32_t* __restrict__ win = cfg->window[rep];
  const int64_t off = (int64_t)rep * n;
  const uint8_t* __restrict__ dones = dones_all + off;
  const uint8_t* __restrict__ ready = ready_all + off;
  const uint8_t* __restrict__ ori_hit = ori_hit_all + off;
  const uint8_t* __restrict__ regression = regression_all + off;
  int64_t now = 0;
  if (lane == 0) {
    now = st->num_timesteps + steps_per_call;
    st->num_timesteps = now;
  }
  const bool words_ok = ((reinterpret_cast<uintptr_t>(dones) | reinterpret_cast<uintptr_t>(ready) | reinterpret_cast<uintptr_t>(ori_hit) |
                          reinterpret_cast<uintptr_t>(regression)) & 3) == 0;   // the flag planes sit at multiples of N inside one buffer
  for (int base = 0; base < n; base += 64 * 64) {
    const int first = base + lane * 64;
    RouteMasks mk = {0ull, 0ull, 0ull, 0ull, 0ull};
    for (int b = 0; b < 64 && first + b < n; b += 4) {
      if (words_ok && first + b + 4 <= n) {   // 4 envs per 32-bit load (the arrays are 256-byte aligned device buffers)
        const unsigned int d4 = *reinterpret_cast<const unsigned int*>(dones + first + b);
        if ((d4 & 0x03030303u) == 0u) continue;
        const unsigned int r4 = *reinterpret_cast<const unsigned int*>(ready + first + b);
        const unsigned int o4 = *reinterpret_cast<const unsigned int*>(ori_hit + first + b);
        const unsigned int g4 = *reinterpret_cast<const unsigned int*>(regression + first + b);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned int d = (d4 >> (8 * k)) & 0xffu;
          if (d & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) {
            const unsigned long long bit = 1ull << (b + k);
            mk.done |= bit;
            if (d & KP1_DONE_SUCCESS) mk.succ |= bit;
            if ((r4 >> (8 * k)) & 0xffu) mk.ready |= bit;
            if ((o4 >> (8 * k)) & 0xffu) mk.ori |= bit;
            if ((g4 >> (8 * k)) & 0xffu) mk.regr |= bit;
          }
        }
      } else {
        for (int k = 0; k < 4 && first + b + k < n; ++k) {
          const uint8_t d = dones[first + b + k];
          if (d & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) {
            const unsigned long long bit = 1ull << (b + k);
            mk.done |= bit;
            if (d & KP1_DONE_SUCCESS) mk.succ |= bit;
            if (ready[first + b + k]) mk.ready |= bit;
            if (ori_hit[first + b + k]) mk.ori |= bit;
            if (regression[first + b + k]) mk.regr |= bit;
          }
        }
      }
    }
    if (__ballot(mk.done != 0ull) == 0ull) continue;
    RouteTrk c = {};
    if (lane == 0) route_trk_load(st, c);
    route_trk_replay(st, win, c, lane, mk, now);
    if (lane == 0) route_trk_store(st, c);
  }
}

// ---- per-step episode records (data parallel) ----------------------------------------------------------------------------------
// The wrapper's flag planes are rewritten by every step, so a chunk of steps cannot be replayed from them: after each step one byte per
// env keeps that step's done bits and the three flags the tracker reads.  Elementwise, 4 envs per lane: 32-bit loads of the done bytes
// and of the three planes (one scalar base, the planes at 32-bit offsets k * N from it), one 32-bit store.
// nonzero byte -> 0x01 in the same byte, for the four bytes of a word at once
__device__ __forceinline__ unsigned int route_bytes_nonzero(unsigned int x) {
  return ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7;
}

__global__ void __launch_bounds__(256) route_episode_records_kernel(const uint8_t* __restrict__ dones, const uint8_t* __restrict__ flags,
                                                                    uint8_t* __restrict__ records, unsigned int n, int words_ok) {
  // flags = the wrapper's byte block: route_ready at [0, N), route_regression at [2N, 3N), orientation_hit at [3N, 4N) (kp1_route_get_info)
  const unsigned int i = (blockIdx.x * 256u + threadIdx.x) * 4u;
  if (i >= n) return;
  if (words_ok) {   // N % 4 == 0 and every base 4-byte aligned: every lane's 4 envs are one aligned word in each array
    const unsigned int d4 = *reinterpret_cast<const unsigned int*>(dones + i);
    const unsigned int r4 = *reinterpret_cast<const unsigned int*>(flags + i);
    const unsigned int g4 = *reinterpret_cast<const unsigned int*>(flags + (2u * n + i));
    const unsigned int o4 = *reinterpret_cast<const unsigned int*>(flags + (3u * n + i));
    *reinterpret_cast<unsigned int*>(records + i) = (d4 & 0x0f0f0f0fu) | (route_bytes_nonzero(r4) << 4) | (route_bytes_nonzero(o4) << 5) |
                                                    (route_bytes_nonzero(g4) << 6);
    return;
  }
  for (unsigned int k = i; k < i + 4u && k < n; ++k)
    records[k] = (uint8_t)((dones[k] & 0x0fu) | (flags[k] ? KP1_ROUTE_REC_READY : 0) | (flags[3u * n + k] ? KP1_ROUTE_REC_ORI_HIT : 0) |
                           (flags[2u * n + k] ? KP1_ROUTE_REC_REGRESSION : 0));
}

// one record word (4 envs starting at bit b of the lane's group) into the lane's masks
__device__ __forceinline__ void route_rec_word(unsigned int w, int b, RouteMasks& mk) {
  if ((w & (0x01010101u * (unsigned)(KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED))) == 0u) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned int d = (w >> (8 * k)) & 0xffu;
    if (d & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) {
      const unsigned long long bit = 1ull << (b + k);
      mk.done |= bit;
      if (d & KP1_DONE_SUCCESS) mk.succ |= bit;
      if (d & KP1_ROUTE_REC_READY) mk.ready |= bit;
      if (d & KP1_ROUTE_REC_ORI_HIT) mk.ori |= bit;
      if (d & KP1_ROUTE_REC_REGRESSION) mk.regr |= bit;
    }
  }
}

// Data-parallel form: `records` = the all-gathered [world][chunk_steps][n_local] record bytes (rank-major).  Replayed step by step and,
// inside a step, rank by rank = global env id order; the clock advances by world * n_local per env step before that step's episodes, as
// the callback's num_timesteps does on one VecEnv of world * n_local envs.  Lane 0 holds the tracker in registers for the whole chunk.
__global__ void __launch_bounds__(64) route_curriculum_chunk_kernel(kp1_route_curriculum_state* __restrict__ st, RouteDevCfg* __restrict__ cfg,
                                                                    const uint8_t* __restrict__ records, int n_local, int chunk_steps, int world) {
  const int lane = threadIdx.x;
  RouteTrk c = {};
  int64_t now = 0;
  if (lane == 0) {
    route_trk_load(st, c);
    now = st->num_timesteps;
  }
  const int64_t per_step = (int64_t)world * n_local;
  for (int t = 0; t < chunk_steps; ++t) {
    now += per_step;
    for (int r = 0; r < world; ++r) {
      const uint8_t* __restrict__ rec = records + ((int64_t)r * chunk_steps + t) * n_local;
      for (int base = 0; base < n_local; base += 64 * 64) {
        const int first = base + lane * 64;
        RouteMasks mk = {0ull, 0ull, 0ull, 0ull, 0ull};
        if (first + 64 <= n_local && (reinterpret_cast<uintptr_t>(rec + first) & 15) == 0) {   // 64 envs in four 16-byte loads
          const uint4* p = reinterpret_cast<const uint4*>(rec + first);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint4 w = p[j];
            route_rec_word(w.x, 16 * j, mk);
            route_rec_word(w.y, 16 * j + 4, mk);
            route_rec_word(w.z, 16 * j + 8, mk);
            route_rec_word(w.w, 16 * j + 12, mk);
          }
        } else {
          for (int b = 0; b < 64 && first + b < n_local; ++b) route_rec_word(rec[first + b], b, mk);
        }
        if (__ballot(mk.done != 0ull) == 0ull) continue;
        route_trk_replay(st, cfg->window[0], c, lane, mk, now);
      }
    }
  }
  if (lane == 0) {
    route_trk_store(st, c);
    st->num_timesteps = now;
  }
}

int route_curriculum_alloc(kp1_route* r, const int32_t* prefix_end_index, int32_t n_stages, double promotion_success_rate,
                           double promotion_route_ready_hit_rate, double promotion_orientation_hit_rate, double promotion_max_regression_rate,
                           int32_t window_episodes, int32_t min_episodes_per_stage, kp1_route_curriculum_state** out_dev);

}  // namespace

extern "C" {

void kp1_route_config_default(kp1_route_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof *c);
#define X(name, dflt) c->reward.name = dflt;
  KP1_ROUTE_REWARD_FIELDS(X)
#undef X
  kp1_route_reset_cfg& s = c->reset;
  s.mode = 0; s.min_route_index = 1; s.max_route_index = 20; s.segment_start_index = 1; s.segment_end_index = 40; s.replay_start_index = 1;
  s.replay_end_index = 120; s.prefix_start_reset_ratio = 0.10; s.random_prefix_reset_ratio = 0.55; s.segment_reset_ratio = 0.20; s.replay_reset_ratio = 0.0;
  s.recovery_reset_ratio = 0.15; s.q_noise_std = 0.002; s.dq_noise_std = 0.0005; s.prev_action_noise_std = 0.02;
  c->include_route_keys = 0; c->sequence_enabled = 0; c->sequence_length = 5; c->reset_ready_streak_on_advance = 1;
}

const char* kp1_route_component_name(int32_t index) {
  static const char* names[KP1_ROUTE_N_COMPONENTS] = {
      "q_goal_progress", "ee_position_progress", "ee_orientation_progress", "route_tangent_progress_bonus", "same_step_route_ready_bonus",
      "route_ready_dwell_bonus", "low_motion_near_waypoint_bonus", "orientation_regression_penalty", "q_route_regression_penalty", "off_route_penalty",
      "action_smoothness_penalty", "dq_penalty", "no_progress_penalty", "curr_q_error", "curr_pos_error", "curr_ori_error", "route_ready"};
  return (index >= 0 && index < KP1_ROUTE_N_COMPONENTS) ? names[index] : nullptr;
}

int kp1_route_create(kp1_env* base, const kp1_route_config* cfg, const double* route_q_host, int32_t n_waypoints, uint64_t seed, uint64_t first_env_id,
                     kp1_route** out) {
  if (!base || !cfg || !route_q_host || !out || n_waypoints < 2) return fail(KP1_ERR_INVALID, "bad argument to kp1_route_create");
  if ((size_t)n_waypoints * NJ * base->real_size() > KP1_ROUTE_MAX_TABLE_LDS_BYTES)
    return fail(KP1_ERR_INVALID, "route too long: the joint table (n_waypoints x 7 reals) must fit 128 KB of LDS (4681 waypoints in fp32, 2340 in fp64)");
  if (base->mode != KP1_MODE_APPROACH) return fail(KP1_ERR_INVALID, "the route wrappers drive an approach-mode base env");
  HIP_TRY(hipSetDevice(base->device));
  kp1_route* r = new kp1_route();
  r->base = base;
  r->n = base->n;
  r->cfg = *cfg;
  r->obs_stride = cfg->include_route_keys ? KP1_ROUTE_OBS_DIM : KP1_OBS_DIM;
  r->n_waypoints = n_waypoints;
  r->n_per_replica = (int32_t)base->n;
  r->win = {cfg->reset.min_route_index, cfg->reset.max_route_index};
  const int64_t n = base->n, W = n_waypoints;
  int rc = KP1_OK;
  auto alloc = [&](void** p, size_t bytes) {
    if (rc != KP1_OK) return;
    if (hipMalloc(p, bytes) != hipSuccess) { rc = fail(KP1_ERR_ALLOC, "hipMalloc failed in kp1_route_create"); return; }
    r->allocs.push_back(*p);
    if (hipMemset(*p, 0, bytes) != hipSuccess) rc = fail(KP1_ERR_NO_DEVICE, "hipMemset failed");
  };
  alloc((void**)&r->q, sizeof(double) * W * NJ);
  alloc((void**)&r->pose, sizeof(double) * W * 6);
  alloc((void**)&r->next_dq, sizeof(double) * W * NJ);
  alloc((void**)&r->progress, sizeof(double) * W);
  alloc((void**)&r->dev_cfg, sizeof(RouteDevCfg));
  alloc((void**)&r->ints, sizeof(int32_t) * 6 * n);
  alloc((void**)&r->bytes, 5 * (size_t)n);
  alloc((void**)&r->reals, base->real_size() * (2 + RP_NUM) * n);
  alloc((void**)&r->rng64, sizeof(uint64_t) * 4 * n);
  alloc((void**)&r->rng32, sizeof(uint32_t) * 2 * n);
  alloc((void**)&r->scratch, sizeof(double) * 4 * NJ * n);
  alloc((void**)&r->opt_scratch, sizeof(double) * 3 * NJ * n);
  alloc((void**)&r->opt_ints, sizeof(int32_t) * 2 * n);
  alloc((void**)&r->base_obs, sizeof(float) * KP1_OBS_DIM * n);
  alloc((void**)&r->base_reward, base->real_size() * n);
  alloc((void**)&r->comps, base->real_size() * KP1_ROUTE_N_COMPONENTS * n);
  if (base->real_type == KP1_REAL_F32) alloc((void**)&r->fused_actions, sizeof(float) * NJ * n);
  if (rc != KP1_OK) { kp1_route_destroy(r); return rc; }
  // load_route_dataset: FK per waypoint on the device in fp64, then path length / tangents / chunks on the host
  r->h_q.assign(route_q_host, route_q_host + W * NJ);
  r->h_pose.resize(W * 6); r->h_next.resize(W * NJ); r->h_progress.resize(W); r->h_chunk.resize(W);
  HIP_TRY(hipMemcpyAsync(r->q, r->h_q.data(), sizeof(double) * W * NJ, hipMemcpyHostToDevice, base->stream));
  rc = kp1_fk_pose6(base->device, KP1_REAL_F64, r->q, r->pose, W, base->stream);
  if (rc != KP1_OK) { kp1_route_destroy(r); return rc; }
  HIP_TRY(hipMemcpyAsync(r->h_pose.data(), r->pose, sizeof(double) * W * 6, hipMemcpyDeviceToHost, base->stream));
  HIP_TRY(hipStreamSynchronize(base->stream));
  double acc = 0.0;
  r->h_progress[0] = 0.0;
  for (int64_t i = 1; i < W; ++i) {
    double s = 0.0;
    for (int k = 0; k < 3; ++k) { const double t = r->h_pose[i * 6 + k] - r->h_pose[(i - 1) * 6 + k]; s += t * t; }
    acc += std::sqrt(s);
    r->h_progress[i] = acc;
  }
  const int mx = (int)W - 1;
  const int lo[7] = {1, 41, 81, 121, 181, 261, 361}, hi[7] = {40, 80, 120, 180, 260, 360, mx};
  for (int64_t i = 0; i < W; ++i) {
    const int64_t nx = i + 1 < W ? i + 1 : W - 1;
    for (int k = 0; k < NJ; ++k) r->h_next[i * NJ + k] = r->h_q[nx * NJ + k] - r->h_q[i * NJ + k];
    int c = 6;
    for (int b = 0; b < 7; ++b) {
      const int h = b < 6 ? (hi[b] < mx ? hi[b] : mx) : mx;
      if (lo[b] <= i && i <= h) { c = b; break; }
    }
    r->h_chunk[i] = c;
  }
  HIP_TRY(hipMemcpyAsync(r->next_dq, r->h_next.data(), sizeof(double) * W * NJ, hipMemcpyHostToDevice, base->stream));
  HIP_TRY(hipMemcpyAsync(r->progress, r->h_progress.data(), sizeof(double) * W, hipMemcpyHostToDevice, base->stream));
  rc = route_upload_cfg(r);
  if (rc == KP1_OK) rc = route_seed_streams(r, seed, first_env_id);
  if (rc != KP1_OK) { kp1_route_destroy(r); return rc; }
  *out = r;
  return KP1_OK;
}

int kp1_route_destroy(kp1_route* r) {
  if (!r) return KP1_OK;
  if (r->base) { (void)hipSetDevice(r->base->device); (void)hipStreamSynchronize(r->base->stream); }
  for (void* p : r->allocs) (void)hipFree(p);
  delete r;
  return KP1_OK;
}

int kp1_route_get_dataset(kp1_route* r, double* poses6, double* progress, double* next_q_delta, int32_t* chunk_id) {
  if (!r) return fail(KP1_ERR_INVALID, "NULL route");
  if (poses6) std::memcpy(poses6, r->h_pose.data(), sizeof(double) * r->h_pose.size());
  if (progress) std::memcpy(progress, r->h_progress.data(), sizeof(double) * r->h_progress.size());
  if (next_q_delta) std::memcpy(next_q_delta, r->h_next.data(), sizeof(double) * r->h_next.size());
  if (chunk_id) std::memcpy(chunk_id, r->h_chunk.data(), sizeof(int32_t) * r->h_chunk.size());
  return KP1_OK;
}

int kp1_route_set_window(kp1_route* r, int32_t min_route_index, int32_t max_route_index) {
  if (!r) return fail(KP1_ERR_INVALID, "NULL route");
  r->cfg.reset.min_route_index = min_route_index;
  r->cfg.reset.max_route_index = max_route_index;
  for (int k = 0; k < r->n_replicas; ++k) {
    r->win[2 * k] = min_route_index;
    r->win[2 * k + 1] = max_route_index;
  }
  return route_upload_cfg(r);
}

int kp1_route_set_replica_window(kp1_route* r, int32_t replica, int32_t min_route_index, int32_t max_route_index) {
  if (!r) return fail(KP1_ERR_INVALID, "NULL route");
  if (replica < 0 || replica >= r->n_replicas) return fail(KP1_ERR_INVALID, "kp1_route_set_replica_window: replica out of range");
  r->win[2 * replica] = min_route_index;
  r->win[2 * replica + 1] = max_route_index;
  return route_upload_cfg(r);
}

int kp1_route_num_replicas(const kp1_route* r) { return r ? r->n_replicas : 0; }

int kp1_route_create_population(kp1_env* base, const kp1_route_config* cfg, const double* route_q_host, int32_t n_waypoints, const uint64_t* seeds,
                                int32_t replicas, kp1_route** out) {
  if (!base || !seeds || !out) return fail(KP1_ERR_INVALID, "bad argument to kp1_route_create_population");
  if (replicas < 1 || replicas > KP1_ROUTE_MAX_REPLICAS || base->n % replicas != 0)
    return fail(KP1_ERR_INVALID, "kp1_route_create_population: replicas must be in [1, KP1_ROUTE_MAX_REPLICAS] and divide the base env's N");
  if (base->real_type != KP1_REAL_F32) return fail(KP1_ERR_UNSUPPORTED, "population route handles drive an f32 base env");
  const int32_t npb = (int32_t)(base->n / replicas);
  kp1_route* r = nullptr;
  int rc = kp1_route_create(base, cfg, route_q_host, n_waypoints, seeds[0], 0, &r);
  if (rc != KP1_OK) return rc;
  r->n_replicas = replicas;
  r->n_per_replica = npb;
  r->win.resize(2 * (size_t)replicas);
  for (int k = 0; k < replicas; ++k) {
    r->win[2 * k] = cfg->reset.min_route_index;
    r->win[2 * k + 1] = cfg->reset.max_route_index;
  }
  rc = route_upload_cfg(r);
  // both streams of env i in block k <- default_rng(seeds[k] + i), the base env's (reset(seed=) semantics of kp1_route_seed) and the wrapper's
  if (rc == KP1_OK) rc = kp1_seed_blocks(base, seeds, replicas, npb);
  if (rc == KP1_OK) rc = seed_planes_by(r->rng64, r->rng32, r->n, base->stream, [=](int64_t i) { return seeds[i / npb] + (uint64_t)(i % npb); });
  if (rc != KP1_OK) { kp1_route_destroy(r); return rc; }
  *out = r;
  return KP1_OK;
}

int kp1_route_seed(kp1_route* r, uint64_t seed, uint64_t first_env_id) {
  if (!r) return fail(KP1_ERR_INVALID, "NULL route");
  int rc = kp1_seed(r->base, seed, first_env_id);  // reset(seed=) also re-seeds the base env's stream
  return rc != KP1_OK ? rc : route_seed_streams(r, seed, first_env_id);
}

int kp1_route_obs_dim(const kp1_route* r) { return r ? (r->cfg.include_route_keys ? KP1_ROUTE_OBS_DIM : KP1_OBS_DIM) : 0; }

int kp1_route_set_obs_stride(kp1_route* r, int32_t stride) {
  if (!r) return fail(KP1_ERR_INVALID, "NULL route handle");
  const int dim = kp1_route_obs_dim(r);
  if (stride < dim || stride > 128 || stride % 4 != 0) return fail(KP1_ERR_INVALID, "obs stride must be >= the observation width, <= 128 and a multiple of 4");
  r->obs_stride = stride;
  return KP1_OK;
}

int kp1_route_reset(kp1_route* r, const uint8_t* mask, const kp1_route_reset_opts* opts, float* obs) {
  if (!r) return fail(KP1_ERR_INVALID, "NULL route");
  kp1_env* e = r->base;
  HIP_TRY(hipSetDevice(e->device));
  const int32_t *ri = nullptr, *si = nullptr;
  const double *q0 = nullptr, *dq0 = nullptr, *pa0 = nullptr;
  int ev = 0;
  if (opts && opts->route_index) {
    ri = opts->route_index; si = opts->start_route_index; q0 = opts->initial_q; dq0 = opts->initial_dq; pa0 = opts->initial_prev_action;
    ev = opts->evaluator_state;
  }
  return with_real(e->real_type, [&](auto real) { return route_launch_reset<decltype(real)>(r, mask, ri, si, q0, dq0, pa0, ev, obs); });
}

int kp1_route_step(kp1_route* r, const void* actions, float* obs, void* reward, uint8_t* done, float* terminal_obs, int32_t auto_reset) {
  if (!r || !actions || !obs || !reward || !done) return fail(KP1_ERR_INVALID, "NULL argument to kp1_route_step");
  HIP_TRY(hipSetDevice(r->base->device));
  return with_real(r->base->real_type, [&](auto real) { return route_launch_step<decltype(real)>(r, actions, obs, reward, done, terminal_obs, auto_reset); });
}

int kp1_route_get_info(kp1_route* r, kp1_route_info_view* out) {
  if (!r || !out) return fail(KP1_ERR_INVALID, "NULL argument");
  const int64_t n = r->base->n;
  out->route_index = r->ints; out->start_route_index = r->ints + n; out->last_route_index = r->ints + 2 * n; out->ready_streak = r->ints + 3 * n;
  out->completed_waypoints = r->ints + 4 * n; out->reset_mode = r->ints + 5 * n;
  out->route_ready = r->bytes; out->waypoint_success = r->bytes + n; out->route_regression = r->bytes + 2 * n; out->orientation_hit = r->bytes + 3 * n;
  out->q_error_norm = r->reals;
  out->nearest_route_q_distance = (const char*)r->reals + r->base->real_size() * n;
  return KP1_OK;
}

int kp1_route_enable_reward_components(kp1_route* r, int32_t enable) {
  if (!r) return fail(KP1_ERR_INVALID, "NULL route");
  r->comps_enabled = enable != 0;
  return KP1_OK;
}
int kp1_route_get_reward_components(kp1_route* r, const void** comps) {
  if (!r || !comps) return fail(KP1_ERR_INVALID, "NULL argument");
  *comps = r->comps;
  return KP1_OK;
}

int kp1_route_rng_get(kp1_route* r, kp1_rng_state* out_host) {
  if (!r || !out_host) return fail(KP1_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(r->base->device));
  return download_rng_planes(r->rng64, r->rng32, out_host, (size_t)r->n, r->base->stream);
}
int kp1_route_rng_set(kp1_route* r, const kp1_rng_state* in_host) {
  if (!r || !in_host) return fail(KP1_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(r->base->device));
  return upload_rng_planes(r->rng64, r->rng32, in_host, (size_t)r->n, r->base->stream);
}

int kp1_route_curriculum_create(kp1_route* r, const int32_t* prefix_end_index, int32_t n_stages, double promotion_success_rate,
                                double promotion_route_ready_hit_rate, double promotion_orientation_hit_rate, double promotion_max_regression_rate,
                                int32_t window_episodes, int32_t min_episodes_per_stage, kp1_route_curriculum_state** out_dev) {
  if (!r || !prefix_end_index || !out_dev) return fail(KP1_ERR_INVALID, "NULL argument");
  if (n_stages < 1 || n_stages > KP1_ROUTE_CURRICULUM_MAX_STAGES) return fail(KP1_ERR_INVALID, "RoutePrefixCurriculumCallback requires 1..16 stages");
  if (window_episodes > KP1_ROUTE_CURRICULUM_MAX_WINDOW) return fail(KP1_ERR_INVALID, "promotion window larger than KP1_ROUTE_CURRICULUM_MAX_WINDOW");
  if (r->n_replicas != 1) return fail(KP1_ERR_UNSUPPORTED, "a population route handle takes kp1_route_curriculum_create_population");
  return route_curriculum_alloc(r, prefix_end_index, n_stages, promotion_success_rate, promotion_route_ready_hit_rate, promotion_orientation_hit_rate,
                                promotion_max_regression_rate, window_episodes, min_episodes_per_stage, out_dev);
}

int kp1_route_curriculum_create_population(kp1_route* r, const int32_t* prefix_end_index, int32_t n_stages, double promotion_success_rate,
                                           double promotion_route_ready_hit_rate, double promotion_orientation_hit_rate,
                                           double promotion_max_regression_rate, int32_t window_episodes, int32_t min_episodes_per_stage,
                                           kp1_route_curriculum_state** out_dev) {
  if (!r || !prefix_end_index || !out_dev) return fail(KP1_ERR_INVALID, "NULL argument");
  if (n_stages < 1 || n_stages > KP1_ROUTE_CURRICULUM_MAX_STAGES) return fail(KP1_ERR_INVALID, "RoutePrefixCurriculumCallback requires 1..16 stages");
  if (window_episodes > KP1_ROUTE_CURRICULUM_MAX_WINDOW) return fail(KP1_ERR_INVALID, "promotion window larger than KP1_ROUTE_CURRICULUM_MAX_WINDOW");
  return route_curriculum_alloc(r, prefix_end_index, n_stages, promotion_success_rate, promotion_route_ready_hit_rate, promotion_orientation_hit_rate,
                                promotion_max_regression_rate, window_episodes, min_episodes_per_stage, out_dev);
}

}  // extern "C"

namespace {
// K = r->n_replicas identical initial trackers in device memory, every window set to the first stage (_on_training_start)
int route_curriculum_alloc(kp1_route* r, const int32_t* prefix_end_index, int32_t n_stages, double promotion_success_rate,
                           double promotion_route_ready_hit_rate, double promotion_orientation_hit_rate, double promotion_max_regression_rate,
                           int32_t window_episodes, int32_t min_episodes_per_stage, kp1_route_curriculum_state** out_dev) {
  const int K = r->n_replicas;
  HIP_TRY(hipSetDevice(r->base->device));
  kp1_route_curriculum_state* h = new kp1_route_curriculum_state();
  std::memset(h, 0, sizeof *h);
  h->window_episodes = window_episodes < 1 ? 1 : window_episodes;
  h->min_episodes_per_stage = min_episodes_per_stage < 1 ? 1 : min_episodes_per_stage;
  h->n_stages = n_stages;
  for (int i = 0; i < n_stages; ++i) h->prefix_end_index[i] = prefix_end_index[i];
  h->promotion_success_rate = promotion_success_rate; h->promotion_route_ready_hit_rate = promotion_route_ready_hit_rate;
  h->promotion_orientation_hit_rate = promotion_orientation_hit_rate; h->promotion_max_regression_rate = promotion_max_regression_rate;
  kp1_route_curriculum_state* d = nullptr;
  if (hipMalloc((void**)&d, sizeof *d * K) != hipSuccess) { delete h; return fail(KP1_ERR_ALLOC, "hipMalloc failed in kp1_route_curriculum_create"); }
  hipError_t e = hipSuccess;
  for (int k = 0; k < K && e == hipSuccess; ++k) e = hipMemcpy(d + k, h, sizeof *h, hipMemcpyHostToDevice);
  delete h;
  if (e != hipSuccess) { (void)hipFree(d); return fail(KP1_ERR_NO_DEVICE, "hipMemcpy failed in kp1_route_curriculum_create"); }
  const int rc = kp1_route_set_window(r, 1, prefix_end_index[0]);   // _on_training_start -> _apply_stage
  if (rc != KP1_OK) { (void)hipFree(d); return rc; }
  r->n_trackers += 1;
  *out_dev = d;
  return KP1_OK;
}
}  // namespace

extern "C" {

int kp1_route_curriculum_destroy(kp1_route* r, kp1_route_curriculum_state* st_dev) {
  if (!r || !st_dev) return KP1_OK;
  (void)hipSetDevice(r->base->device);
  (void)hipStreamSynchronize(r->base->stream);
  (void)hipFree(st_dev);
  if (r->n_trackers > 0) r->n_trackers -= 1;
  return KP1_OK;
}

int kp1_route_curriculum_observe(kp1_route* r, kp1_route_curriculum_state* st_dev, const uint8_t* dones, int32_t steps_per_call, void* stream) {
  if (!r || !st_dev || !dones) return fail(KP1_ERR_INVALID, "bad argument to kp1_route_curriculum_observe");
  if (r->n_replicas != 1) return fail(KP1_ERR_UNSUPPORTED, "a population route handle takes kp1_route_curriculum_observe_population");
  const int64_t n = r->base->n;
  return launch_env(route_curriculum_kernel, 64, 64, 0, (hipStream_t)stream, st_dev, r->dev_cfg, dones, r->bytes, r->bytes + 3 * n, r->bytes + 2 * n, (int)n,
                    (int)steps_per_call);
}

int kp1_route_episode_records(kp1_route* r, const uint8_t* dones, uint8_t* records, void* stream) {
  if (!r || !dones || !records) return fail(KP1_ERR_INVALID, "NULL argument to kp1_route_episode_records");
  const int64_t n = r->base->n;
  if (n > (int64_t)(UINT32_MAX / 4u)) return fail(KP1_ERR_INVALID, "kp1_route_episode_records: N too large for 32-bit plane offsets");
  const int words_ok = (n % 4 == 0) && ((reinterpret_cast<uintptr_t>(dones) | reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(r->bytes)) & 3) == 0;
  return launch_env(route_episode_records_kernel, (n + 3) / 4, UTIL_BLOCK, 0, (hipStream_t)stream, dones, r->bytes, records, (unsigned int)n, words_ok);   // 4 envs per lane
}

int kp1_route_curriculum_observe_chunk(kp1_route* r, kp1_route_curriculum_state* st_dev, const uint8_t* records, int32_t n_local, int32_t chunk_steps,
                                       int32_t world, void* stream) {
  if (!r || !st_dev || !records || n_local <= 0 || chunk_steps <= 0 || world <= 0)
    return fail(KP1_ERR_INVALID, "bad argument to kp1_route_curriculum_observe_chunk");
  if (r->n_replicas != 1) return fail(KP1_ERR_UNSUPPORTED, "the data-parallel chunk tracker has no population form");
  return launch_env(route_curriculum_chunk_kernel, 64, 64, 0, (hipStream_t)stream, st_dev, r->dev_cfg, records, (int)n_local, (int)chunk_steps, (int)world);
}

int kp1_route_curriculum_read(kp1_route* r, const kp1_route_curriculum_state* st_dev, kp1_route_curriculum_state* out_host, void* stream) {
  if (!r || !st_dev || !out_host) return fail(KP1_ERR_INVALID, "NULL argument");
  HIP_TRY(hipMemcpyAsync(out_host, st_dev, sizeof *out_host, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  // promotions rewrote the window in the device copy of the route config: keep the host copy (re-uploaded by later setters) in step
  r->cfg.reset.min_route_index = 1;
  r->cfg.reset.max_route_index = out_host->prefix_end_index[out_host->stage_index];
  r->win[0] = r->cfg.reset.min_route_index;
  r->win[1] = r->cfg.reset.max_route_index;
  return KP1_OK;
}

int kp1_route_curriculum_observe_population(kp1_route* r, kp1_route_curriculum_state* st_dev, const uint8_t* dones, int32_t steps_per_call, void* stream) {
  if (!r || !st_dev || !dones) return fail(KP1_ERR_INVALID, "bad argument to kp1_route_curriculum_observe_population");
  const int64_t n = r->base->n;
  return launch_env(route_curriculum_kernel, 64 * r->n_replicas, 64, 0, (hipStream_t)stream, st_dev, r->dev_cfg, dones, r->bytes, r->bytes + 3 * n,
                    r->bytes + 2 * n, (int)r->n_per_replica, (int)steps_per_call);   // one wave per tracker
}

int kp1_route_curriculum_read_replica(kp1_route* r, const kp1_route_curriculum_state* st_dev, int32_t replica, kp1_route_curriculum_state* out_host,
                                      void* stream) {
  if (!r || !st_dev || !out_host) return fail(KP1_ERR_INVALID, "NULL argument");
  if (replica < 0 || replica >= r->n_replicas) return fail(KP1_ERR_INVALID, "kp1_route_curriculum_read_replica: replica out of range");
  HIP_TRY(hipMemcpyAsync(out_host, st_dev + replica, sizeof *out_host, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  r->win[2 * replica] = 1;
  r->win[2 * replica + 1] = out_host->prefix_end_index[out_host->stage_index];
  if (r->n_replicas == 1) {
    r->cfg.reset.min_route_index = 1;
    r->cfg.reset.max_route_index = r->win[1];
  }
  return KP1_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- chained sequential evaluation
// evaluate_sequential_route (route_curriculum.py, _roll_one) for every row of a handle at once.  After the unchanged route step
// (auto_reset = 0) kp1_route_chain_kernel, one lane per row, does what the evaluator's host loop does between two steps: the per-episode
// bookkeeping from the planes the step has just written, and at the end of an episode the record of the waypoint and the explicit-state reset
// to the next one (route_reset_env from the row's own q / dq / prev_action, read as get_state reads them).  Nothing here draws from a PCG64
// stream: an explicit-state reset with a goal takes no branch of reset_env that loads one.
namespace {

// RouteChainDev, RouteChainArgs and route_chain_open: kp1_route_step.inc (kp1_mlp.hip runs the chain step inside its one-launch kernel too)
template <typename R>
__global__ void __launch_bounds__(64) kp1_route_chain_begin_kernel(const EnvState<R> st, const RouteChainDev ch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= st.n) return;
  route_chain_open<R>(st, ch, i, ch.start[i]);
  ch.n_records[i] = 0;
  ch.alive[i] = 1;
  if (i == 0) *ch.n_alive = (int32_t)st.n;
}

template <typename R>
__global__ void __launch_bounds__(64) kp1_route_chain_kernel(const RouteChainArgs<R> a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const EnvState<R>& st = a.st;
  const RouteChainDev& ch = a.ch;
  int alive_after = 0;
  if (i < st.n) {
#include "kp1_route_chain_body.inc"
  }
  const unsigned long long bal = __ballot(alive_after != 0);
  if (threadIdx.x == 0 && bal) atomicAdd(ch.n_alive, __popcll(bal));
}

}  // namespace

// struct kp1_route_chain: kp1_route_host.hpp

namespace kp1 {
// what a chain cannot run on; text for kp1_last_error, or nullptr (declared in kp1_host.hpp: kp1_mlp.hip asks too)
const char* route_chain_refusal(const kp1_route* r) {
  if (r->base->real_type != KP1_REAL_F32) return "a route chain drives an f32 base env (the f64 handle keeps the host evaluator)";
  if (r->cfg.sequence_enabled) return "a route chain runs the single-waypoint wrapper: the handle has route.sequence enabled";
  if (r->comps_enabled) return "a route chain does not record reward components (kp1_route_enable_reward_components is on)";
  if (r->n_trackers > 0) return "a route chain cannot run on a handle with a prefix curriculum tracker attached";
  return nullptr;
}
}  // namespace kp1
using kp1::route_chain_refusal;

extern "C" {

int kp1_route_chain_create(kp1_route* r, const int32_t* start_host, const int32_t* end_host, int32_t n_rows, int32_t stop_on_failure,
                           kp1_route_chain** out) {
  if (!r || !start_host || !end_host || !out) return fail(KP1_ERR_INVALID, "NULL argument to kp1_route_chain_create");
  if (const char* why = route_chain_refusal(r)) return fail(KP1_ERR_UNSUPPORTED, why);
  if ((int64_t)n_rows != r->base->n) return fail(KP1_ERR_INVALID, "kp1_route_chain_create: n_rows must equal the handle's env count");
  int max_len = 0;
  for (int32_t i = 0; i < n_rows; ++i) {
    if (start_host[i] < 1) return fail(KP1_ERR_INVALID, "kp1_route_chain_create: start_index < 1");
    if (end_host[i] < start_host[i]) return fail(KP1_ERR_INVALID, "kp1_route_chain_create: end_index < start_index");
    if (end_host[i] >= r->n_waypoints) return fail(KP1_ERR_INVALID, "kp1_route_chain_create: end_index >= n_waypoints");
    max_len = std::max(max_len, (int)(end_host[i] - start_host[i] + 1));
  }
  HIP_TRY(hipSetDevice(r->base->device));
  kp1_route_chain* c = new kp1_route_chain();
  c->n_rows = n_rows;
  c->owner = r;
  const size_t n = (size_t)n_rows;
  int rc = KP1_OK;
  auto alloc = [&](void** p, size_t bytes) {
    if (rc != KP1_OK) return;
    if (hipMalloc(p, bytes) != hipSuccess) { rc = fail(KP1_ERR_ALLOC, "hipMalloc failed in kp1_route_chain_create"); return; }
    c->allocs.push_back(*p);
    if (hipMemset(*p, 0, bytes) != hipSuccess) rc = fail(KP1_ERR_NO_DEVICE, "hipMemset failed");
  };
  int32_t* ints = nullptr;     // start, end, wp, steps, first_ready, max_streak, n_records, zeros, n_alive
  float* mins = nullptr;
  alloc((void**)&ints, sizeof(int32_t) * (8 * n + 1));
  alloc((void**)&mins, sizeof(float) * 3 * n);
  alloc((void**)&c->d.alive, n);
  alloc((void**)&c->d.records, sizeof(kp1_route_chain_record) * n * (size_t)max_len);
  alloc((void**)&c->init_q, sizeof(double) * NJ * n);
  if (rc != KP1_OK) { kp1_route_chain_destroy(r, c); return rc; }
  c->d.start = ints; c->d.end = ints + n; c->d.wp = ints + 2 * n; c->d.steps = ints + 3 * n; c->d.first_ready = ints + 4 * n;
  c->d.max_streak = ints + 5 * n; c->d.n_records = ints + 6 * n; c->zeros = ints + 7 * n; c->d.n_alive = ints + 8 * n;
  c->d.min_pos = mins; c->d.min_ori = mins + n; c->d.min_q = mins + 2 * n;
  c->d.max_len = max_len; c->d.stop_on_failure = stop_on_failure != 0;
  std::vector<double> q0(NJ * n);
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < NJ; ++k) q0[i * NJ + k] = r->h_q[(size_t)(start_host[i] - 1) * NJ + k];
  if (hipMemcpy(ints, start_host, sizeof(int32_t) * n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(ints + n, end_host, sizeof(int32_t) * n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->init_q, q0.data(), sizeof(double) * NJ * n, hipMemcpyHostToDevice) != hipSuccess) {
    kp1_route_chain_destroy(r, c);
    return fail(KP1_ERR_NO_DEVICE, "hipMemcpy failed in kp1_route_chain_create");
  }
  c->counted = true;
  r->n_chains += 1;
  *out = c;
  return KP1_OK;
}

int kp1_route_chain_destroy(kp1_route* r, kp1_route_chain* c) {
  if (!c) return KP1_OK;
  if (r && c->counted && r->n_chains > 0) r->n_chains -= 1;
  if (r && r->base) { (void)hipSetDevice(r->base->device); (void)hipStreamSynchronize(r->base->stream); }
  for (void* p : c->allocs) (void)hipFree(p);
  delete c;
  return KP1_OK;
}

int kp1_route_chain_begin(kp1_route* r, kp1_route_chain* c, float* obs) {
  if (!r || !c || !obs) return fail(KP1_ERR_INVALID, "NULL argument to kp1_route_chain_begin");
  if (const char* why = route_chain_refusal(r)) return fail(KP1_ERR_UNSUPPORTED, why);
  if ((int64_t)c->n_rows != r->base->n) return fail(KP1_ERR_INVALID, "kp1_route_chain_begin: the chain was created for another env count");
  kp1_env* e = r->base;
  HIP_TRY(hipSetDevice(e->device));
  const int rc = route_launch_reset<float>(r, nullptr, c->d.start, c->zeros, c->init_q, nullptr, nullptr, 1, obs);
  if (rc != KP1_OK) return rc;
  return launch_env(kp1_route_chain_begin_kernel<float>, e->n, ENV_BLOCK, 0, e->stream, state_of<float>(e), c->d);
}

int kp1_route_chain_step(kp1_route* r, kp1_route_chain* c, const float* actions, float* obs, float* reward, uint8_t* done, int32_t* tags) {
  if (!r || !c || !actions || !obs || !reward || !done) return fail(KP1_ERR_INVALID, "NULL argument to kp1_route_chain_step");
  if (const char* why = route_chain_refusal(r)) return fail(KP1_ERR_UNSUPPORTED, why);
  if ((int64_t)c->n_rows != r->base->n) return fail(KP1_ERR_INVALID, "kp1_route_chain_step: the chain was created for another env count");
  kp1_env* e = r->base;
  HIP_TRY(hipSetDevice(e->device));
  const int rc = route_launch_step<float>(r, actions, obs, reward, done, nullptr, 0);
  if (rc != KP1_OK) return rc;
  HIP_TRY(hipMemsetAsync(c->d.n_alive, 0, sizeof(int32_t), e->stream));
  RouteChainArgs<float> a;
  fill_route_args<float>(a, r, obs);
  a.ch = c->d; a.done = done; a.tags = tags;
  return launch_env(kp1_route_chain_kernel<float>, e->n, ENV_BLOCK, 0, e->stream, a);
}

int kp1_route_chain_get_view(kp1_route_chain* c, kp1_route_chain_view* out) {
  if (!c || !out) return fail(KP1_ERR_INVALID, "NULL argument to kp1_route_chain_get_view");
  out->records = c->d.records; out->n_records = c->d.n_records; out->n_alive = c->d.n_alive;
  out->n_rows = c->n_rows; out->max_len = c->d.max_len;
  return KP1_OK;
}

}  // extern "C"
