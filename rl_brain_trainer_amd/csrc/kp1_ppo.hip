// kp1_ppo.hip -- PPO-side device kernels (include/kp1_ppo.h): GAE scan, time-limit bootstrap, epoch permutation and per-minibatch advantage
// statistics, device-resident curriculum tracker, training monitor with explained variance.  The actor-critic MLP kernels live in kp1_mlp.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/kp1_ppo.h"
#include "kp1_host.hpp"

using kp1::fail;
using kp1::use_device;

namespace {

// One lane per env; every [t] row access is a fully coalesced wave instruction (4 B/lane f32, 1 B/lane done).
// Algorithmic traffic: read r, V, done (9 B) + write A, R (8 B) per sample.
__device__ __forceinline__ void gae_column(const float* __restrict__ rewards, const float* __restrict__ values, const uint8_t* __restrict__ dones,
                                           const float* __restrict__ last_values, float gamma, float lam, float* __restrict__ adv,
                                           float* __restrict__ ret, int T, int N, int i) {
  float next_value = last_values[i];
  float last_gae = 0.0f;
  // prefetch-friendly reverse walk; T is small (<= a few thousand)
  for (int t = T - 1; t >= 0; --t) {
    const int64_t k = (int64_t)t * N + i;
    const float nonterm = (dones[k] & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) ? 0.0f : 1.0f;
    const float v = values[k];
    const float delta = rewards[k] + gamma * next_value * nonterm - v;
    last_gae = delta + gamma * lam * nonterm * last_gae;
    adv[k] = last_gae;
    ret[k] = last_gae + v;
    next_value = v;
  }
}

__global__ void __launch_bounds__(256) gae_scan_kernel(const float* __restrict__ rewards, const float* __restrict__ values,
                                                       const uint8_t* __restrict__ dones, const float* __restrict__ last_values,
                                                       float gamma, float lam, float* __restrict__ adv, float* __restrict__ ret, int T, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  gae_column(rewards, values, dones, last_values, gamma, lam, adv, ret, T, N, i);
}

// gae_scan_kernel with (gamma, lambda) of column i's replica read from gamma_lambda [K][2]: the same gae_column, so a column computes bit for
// bit what the single scan computes with its replica's two scalars
__global__ void __launch_bounds__(256) gae_scan_replicas_kernel(const float* __restrict__ rewards, const float* __restrict__ values,
                                                                const uint8_t* __restrict__ dones, const float* __restrict__ last_values,
                                                                const float* __restrict__ gamma_lambda, int n_per_replica, float* __restrict__ adv,
                                                                float* __restrict__ ret, int T, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int r = i / n_per_replica;
  gae_column(rewards, values, dones, last_values, gamma_lambda[2 * r], gamma_lambda[2 * r + 1], adv, ret, T, N, i);
}

__global__ void __launch_bounds__(256) bootstrap_kernel(float* __restrict__ rewards, const float* __restrict__ tv,
                                                        const uint8_t* __restrict__ dones, float gamma, int64_t count) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint8_t d = dones[k];
  if ((d & KP1_DONE_TRUNCATED) && !(d & KP1_DONE_TERMINATED)) rewards[k] += gamma * tv[k];
}

// PointCurriculumCallback._on_step; callbacks.py:71-92.  One wave.  Each lane loads 64 consecutive done bytes (4 x 16 B)
// and condenses them into a 64-bit done mask and a success mask, so 4096 envs cost one round of loads; a ballot skips
// the common case where no episode ended.  Finished episodes are then replayed strictly in env order by lane 0 (the masks
// of lane k are fetched with a shuffle), which is what the reference's sequential scan does.
//
// [r2] The tracker's state lives in registers and its success ring in LDS for the whole launch (TrackerCtx): round 2's profile had this
// one-wave kernel at 13.2 us per env step (3 % of the PPO iteration) because lane 0 replayed ~45 finished episodes per step with every
// field of *st re-read from global memory after every ring store (the compiler must assume the ring aliases them) -- a chain of
// dependent memory round trips -- and, below the last stage, re-summed the whole ring per episode.  The window sum is now carried along
// (sum += new - overwritten: the same integer the reference's sum(window) gives), so an episode costs a few LDS / scalar instructions.
struct TrackerCtx {
  int stage, count, len, head, window, min_episodes, max_stage, n_events, sum;
  double threshold;
  long long timesteps;
  bool ring_dirty;
};

__device__ __forceinline__ void tracker_load(const kp1_curriculum_state* __restrict__ st, int* __restrict__ ring, TrackerCtx& c) {
  const int lane = threadIdx.x;
  c.stage = st->stage_index; c.count = st->stage_episode_count; c.len = st->ring_len; c.head = st->ring_head;
  c.window = st->window_episodes; c.min_episodes = st->min_episodes_per_stage; c.max_stage = st->max_stage_index; c.n_events = st->n_events;
  c.threshold = st->success_rate_threshold; c.timesteps = st->num_timesteps;
  c.ring_dirty = false;
  // live entries: the len positions from head on (while the ring is filling head is 0; once full every entry is live)
  int part = 0;
  for (int k = lane; k < c.window; k += 64) {
    const int v = st->ring[k];
    ring[k] = v;
    const int age = k >= c.head ? k - c.head : k - c.head + c.window;
    if (age < c.len) part += v;
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  c.sum = part;
  __syncthreads();
}

__device__ __forceinline__ void tracker_store(kp1_curriculum_state* __restrict__ st, const int* __restrict__ ring, const TrackerCtx& c) {
  const int lane = threadIdx.x;
  __syncthreads();
  if (c.ring_dirty)
    for (int k = lane; k < c.window; k += 64) st->ring[k] = ring[k];
  if (lane == 0) {
    st->stage_index = c.stage; st->stage_episode_count = c.count; st->ring_len = c.len; st->ring_head = c.head;
    st->n_events = c.n_events; st->num_timesteps = c.timesteps;
  }
}

// [r3] Many episodes in one block of 4096 envs (every env of a handle truncates in the same step when the episodes started together: 4096
// finished episodes at once, which lane 0 replayed in ~600 us -- 1.4 % of the benchmark's iteration hidden in a "4.7 us" kernel).  Same result,
// computed by the whole wave: the success bits in episode order go to LDS, a prefix count over (window contents ++ new bits) gives the window
// sum after EVERY episode at once, the first episode that satisfies the promotion rule is a wave-min, and the ring / length / head / sum after
// appending a run of episodes follow in closed form (entry j of a run lands in slot (head + len + j) mod window, full or not).  A promotion
// empties the window and the search continues behind it.  Wave-uniform in, wave-uniform out; LDS scratch: 4096 bits-as-bytes + prefix counts.
// TRK_PARALLEL_MIN: finished episodes per 4096-env block from which the whole-wave path is taken
constexpr int TRK_BLOCK = 64 * 64, TRK_PARALLEL_MIN = 192;
struct TrackerScratch { uint8_t* sbit; uint16_t* pfx; };

// append episodes [pos, pos + R) of sbit to the window; no promotion check
__device__ __forceinline__ void tracker_append_run(int* __restrict__ ring, TrackerCtx& c, const uint8_t* __restrict__ sbit, int pos, int R) {
  const int lane = threadIdx.x, W = c.window;
  const int j0 = R > W ? R - W : 0;                       // earlier entries of the run are overwritten by later ones
  __syncthreads();
  for (int j = j0 + lane; j < R; j += 64) ring[(c.head + c.len + j) % W] = sbit[pos + j];
  __syncthreads();
  const int over = c.len + R - W;
  c.head = over > 0 ? (c.head + over) % W : c.head;
  c.len = c.len + R < W ? c.len + R : W;
  c.count += R;
  int part = 0;
  for (int k = lane; k < W; k += 64) {
    const int age = k >= c.head ? k - c.head : k - c.head + W;
    if (age < c.len) part += ring[k];
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  c.sum = part;
}

__device__ __forceinline__ void tracker_block_parallel(kp1_curriculum_state* __restrict__ st, int* __restrict__ ring, TrackerCtx& c, const TrackerScratch& ws,
                                                       unsigned long long dmask, unsigned long long smask, int E) {
  const int lane = threadIdx.x, W = c.window;
  // success bits in episode (= env) order
  int mine = __popcll(dmask), off = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(off, d);
    if (lane >= d) off += up;
  }
  off -= mine;                                            // exclusive prefix: index of this lane's first finished episode
  __syncthreads();
  for (unsigned long long m = dmask; m; m &= m - 1) {
    const int b = __ffsll((long long)m) - 1;
    ws.sbit[off++] = (uint8_t)((smask >> b) & 1ull);
  }
  __syncthreads();
  int pos = 0;
  while (pos < E) {
    const int R = E - pos;
    if (c.stage >= c.max_stage) {                          // last stage: the window only records
      tracker_append_run(ring, c, ws.sbit, pos, R);
      break;
    }
    // prefix counts Q[0 .. L + R] over Y = (window contents, oldest first) ++ sbit[pos ..): Q[j] = successes among the first j entries of Y
    const int L = c.len, T = L + R;
    const int seg = (T + 63) / 64, j_lo = lane * seg < T ? lane * seg : T, j_hi = j_lo + seg < T ? j_lo + seg : T;
    auto y = [&](int j) -> int { return j < L ? ring[(c.head + j) % W] : (int)ws.sbit[pos + (j - L)]; };
    int tot = 0;
    for (int j = j_lo; j < j_hi; ++j) tot += y(j);
    int run = tot;
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(run, d);
      if (lane >= d) run += up;
    }
    run -= tot;
    __syncthreads();
    if (lane == 0) ws.pfx[0] = 0;
    for (int j = j_lo; j < j_hi; ++j) {
      run += y(j);
      ws.pfx[j + 1] = (uint16_t)run;
    }
    __syncthreads();
    // first episode r of the run after whose append the rule holds: count + r + 1 >= min_episodes, window full, rate >= threshold
    int best = R;
    for (int r = lane; r < R; r += 64) {
      const int filled = L + r + 1;
      if (filled < W || c.count + r + 1 < c.min_episodes) continue;
      const int wsum = (int)ws.pfx[filled] - (int)ws.pfx[filled - W];
      if ((double)wsum / (double)W >= c.threshold) {
        best = r;
        break;                                            // r only grows along this lane's stride
      }
    }
    for (int d = 32; d > 0; d >>= 1) {
      const int o = __shfl_xor(best, d);
      best = o < best ? o : best;
    }
    if (best >= R) {                                       // no promotion inside this run
      tracker_append_run(ring, c, ws.sbit, pos, R);
      break;
    }
    const int filled = L + best + 1;
    const double rate = (double)((int)ws.pfx[filled] - (int)ws.pfx[filled - W]) / (double)W;
    if (lane == 0 && c.n_events < KP1_CURRICULUM_MAX_HISTORY) {
      kp1_curriculum_event& ev = st->events[c.n_events];
      ev.total_timesteps = c.timesteps;
      ev.from_stage = c.stage;
      ev.to_stage = c.stage + 1;
      ev.trigger_success_rate = rate;
    }
    c.n_events += 1;
    c.stage += 1;
    c.count = 0;
    c.len = 0;
    c.head = 0;
    c.sum = 0;
    pos += best + 1;
  }
}

// consume dones[0 .. n) in index order.  c is wave-uniform on entry and on exit (lane 0's values are broadcast at the end).
__device__ __forceinline__ void curriculum_scan(kp1_curriculum_state* __restrict__ st, int* __restrict__ ring, TrackerCtx& c, const TrackerScratch& ws,
                                                const uint8_t* __restrict__ dones, int n, int steps_per_call) {
  const int lane = threadIdx.x;
  c.timesteps += steps_per_call;
  for (int base = 0; base < n; base += 64 * 64) {
    const int first = base + lane * 64;
    unsigned long long dmask = 0ull, smask = 0ull;
    if (first + 64 <= n && (reinterpret_cast<uintptr_t>(dones + first) & 15) == 0) {
      const uint4* p = reinterpret_cast<const uint4*>(dones + first);
      uint4 w[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) w[q] = p[q];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned int words[4] = {w[q].x, w[q].y, w[q].z, w[q].w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const unsigned int d = (words[k] >> (8 * b)) & 0xffu;
            const int bit = q * 16 + k * 4 + b;
            if (d & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) {
              dmask |= 1ull << bit;
              if (d & KP1_DONE_SUCCESS) smask |= 1ull << bit;
            }
          }
      }
    } else {
      for (int b = 0; b < 64 && first + b < n; ++b) {
        const uint8_t d = dones[first + b];
        if (d & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) {
          dmask |= 1ull << b;
          if (d & KP1_DONE_SUCCESS) smask |= 1ull << b;
        }
      }
    }
    unsigned long long busy = __ballot(dmask != 0ull);
    if (busy == 0ull) continue;
    c.ring_dirty = true;
    {
      int ended = __popcll(dmask);
      for (int off = 32; off > 0; off >>= 1) ended += __shfl_xor(ended, off);
      if (ended >= TRK_PARALLEL_MIN) {                     // wave-uniform
        tracker_block_parallel(st, ring, c, ws, dmask, smask, ended);
        continue;
      }
    }
    // the replay's prologue; the limits are copied here, in front of the loop: inside the lane-0 branch they move the listing
    int stage = c.stage, count = c.count, len = c.len, head = c.head, sum = c.sum, n_events = c.n_events;
    const int window = c.window, max_stage = c.max_stage, min_episodes = c.min_episodes;
    const double threshold = c.threshold;
    const long long timesteps = c.timesteps;
    constexpr bool TRK_STORES_STAGE = false;               // tracker_store writes the stage when the scan is over
    while (busy) {   // lanes that saw a finished episode, in lane (= env) order
      const int src = __ffsll((long long)busy) - 1;
      busy &= busy - 1;
      unsigned long long m = __shfl(dmask, src);
      const unsigned long long sm = __shfl(smask, src);
      if (lane != 0) continue;
#include "kp1_tracker_replay_body.inc"
    }
    c.stage = __shfl(stage, 0); c.count = __shfl(count, 0); c.len = __shfl(len, 0); c.head = __shfl(head, 0);
    c.sum = __shfl(sum, 0); c.n_events = __shfl(n_events, 0);
  }
}

__global__ void __launch_bounds__(64) curriculum_kernel(kp1_curriculum_state* __restrict__ st, const uint8_t* __restrict__ dones, int n,
                                                        int steps_per_call) {
#include "kp1_tracker_scratch.inc"
#include "kp1_tracker_step_body.inc"
}

// Data-parallel rollouts exchange the done bytes once per CHUNK of env steps instead of once per step: `dones` is the all-gathered
// [world][chunk_steps][n_local] block (rank-major, as all_gather_into_tensor lays it out).  The tracker replays it in the order the
// reference callback would have seen a single VecEnv of world * n_local envs: step by step, and inside a step rank by rank = global
// env id order (callbacks.py:78-91).  One wave; the state stays in registers / LDS across the whole chunk.
__global__ void __launch_bounds__(64) curriculum_chunk_kernel(kp1_curriculum_state* __restrict__ st, const uint8_t* __restrict__ dones, int n_local,
                                                              int chunk_steps, int world, int steps_per_env_step) {
#include "kp1_tracker_scratch.inc"
  TrackerCtx c;
  tracker_load(st, ring, c);
  for (int t = 0; t < chunk_steps; ++t)
    for (int r = 0; r < world; ++r)
      curriculum_scan(st, ring, c, ws, dones + ((int64_t)r * chunk_steps + t) * n_local, n_local, r == 0 ? steps_per_env_step : 0);
  tracker_store(st, ring, c);
}

// K trackers in one launch (kp1_curriculum_observe_population): workgroup k is curriculum_kernel on tracker k and the done bytes
// [k n, (k + 1) n) of its replica, early-out included: both include the same step body.
__global__ void __launch_bounds__(64) curriculum_population_kernel(kp1_curriculum_state* __restrict__ states, const uint8_t* __restrict__ dones_all,
                                                                   int n, int steps_per_call) {
#include "kp1_tracker_scratch.inc"
  kp1_curriculum_state* __restrict__ st = states + blockIdx.x;
  const uint8_t* __restrict__ dones = dones_all + (int64_t)blockIdx.x * n;
#include "kp1_tracker_step_body.inc"
}

// The one launch of this file: `blocks` workgroups of `block` lanes (every grid here is one-dimensional and no kernel takes dynamic LDS), then the
// launch check of kp1_host.hpp.  kp1_env.hip's launch_env derives its grid from a lane count and passes LDS bytes; half the sites here state a
// workgroup count (one per tracker, replica or minibatch), so each unit keeps its own five lines.
template <typename... Params, typename... Args>
int launch(void (*kernel)(Params...), int64_t blocks, int block, void* stream, const Args&... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3((unsigned)block), 0, (hipStream_t)stream, args...);
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}

// lanes per workgroup of the two GAE scans (one lane per env column): one wave per workgroup up to 16384 columns, four beyond
constexpr int gae_block(int N) { return N <= 16384 ? 64 : 256; }

}  // namespace

extern "C" {

int kp1_gae_scan(int32_t device, const float* rewards, const float* values, const uint8_t* dones, const float* last_values, float gamma,
                 float gae_lambda, float* advantages, float* returns, int32_t T, int32_t N, void* stream) {
  if (!rewards || !values || !dones || !last_values || !advantages || !returns || T <= 0 || N <= 0) return fail(KP1_ERR_INVALID, "bad argument to kp1_gae_scan");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  const int block = gae_block(N);
  return launch(gae_scan_kernel, (N + block - 1) / block, block, stream, rewards, values, dones, last_values, gamma, gae_lambda, advantages, returns, T, N);
}

int kp1_gae_scan_replicas(int32_t device, const float* rewards, const float* values, const uint8_t* dones, const float* last_values,
                          const float* gamma_lambda, int32_t n_per_replica, float* advantages, float* returns, int32_t T, int32_t N, void* stream) {
  if (!rewards || !values || !dones || !last_values || !gamma_lambda || !advantages || !returns || T <= 0 || N <= 0)
    return fail(KP1_ERR_INVALID, "bad argument to kp1_gae_scan_replicas");
  if (n_per_replica <= 0 || N % n_per_replica != 0) return fail(KP1_ERR_INVALID, "kp1_gae_scan_replicas: N must be a multiple of n_per_replica");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  const int block = gae_block(N);
  return launch(gae_scan_replicas_kernel, (N + block - 1) / block, block, stream, rewards, values, dones, last_values, gamma_lambda, n_per_replica,
                advantages, returns, T, N);
}

}  // extern "C"

namespace {
// (sum, sum of squares) of the advantages of every minibatch of an epoch in one launch: block b covers
// idx[b * mb .. min((b + 1) * mb, total)).  fp64, fixed summation order => deterministic.
__global__ void __launch_bounds__(256) adv_minibatch_sums_kernel(const float* __restrict__ adv, const int64_t* __restrict__ idx, int64_t total, int64_t mb,
                                                                 double* __restrict__ out) {
  __shared__ double s1[256], s2[256];
  const int64_t begin = (int64_t)blockIdx.x * mb, end = begin + mb < total ? begin + mb : total;
  double a = 0.0, b = 0.0;
  for (int64_t i = begin + threadIdx.x; i < end; i += 256) {
    const double v = (double)adv[idx ? idx[i] : i];
    a += v;
    b += v * v;
  }
  s1[threadIdx.x] = a;
  s2[threadIdx.x] = b;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) {
      s1[threadIdx.x] += s1[threadIdx.x + k];
      s2[threadIdx.x] += s2[threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[3 * blockIdx.x] = s1[0];
    out[3 * blockIdx.x + 1] = s2[0];
    out[3 * blockIdx.x + 2] = (double)(end - begin);
  }
}
// keyed bijection on [0, 2^bits): every round is invertible modulo 2^bits (odd multiplier; x ^= x >> s with s >= 1), so the composition is
// a permutation; multiplication carries low bits upward, the xorshift carries high bits downward.  Cycle walking restricts it to [0, n).
struct PermKeys { uint32_t mul[4], add[4]; };
__global__ void __launch_bounds__(256) permutation_kernel(int64_t* __restrict__ out, int64_t n, int bits, const PermKeys k) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t mask = bits >= 32 ? 0xffffffffu : ((1u << bits) - 1u);
  const int sh = bits > 1 ? bits / 2 : 1;
  uint32_t x = (uint32_t)i;
  do {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      x = (x * k.mul[r] + k.add[r]) & mask;
      x ^= x >> sh;
    }
  } while ((int64_t)x >= n);
  out[i] = (int64_t)x;
}

// (sum, sum of squares, count) -> (mean, 1 / (unbiased std + 1e-8)); f64 arithmetic in the order of the torch expressions it replaces
__global__ void __launch_bounds__(64) adv_minibatch_stats_kernel(const double* __restrict__ sums, int64_t n_mb, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= n_mb) return;
  const double s0 = sums[3 * b], s1 = sums[3 * b + 1], cnt = sums[3 * b + 2];
  const double mean = s0 / cnt;
  const double dof = cnt - 1.0 < 1.0 ? 1.0 : cnt - 1.0;
  double var = (s1 - cnt * mean * mean) / dof;
  var = var < 0.0 ? 0.0 : var;
  out[2 * b] = (float)mean;
  out[2 * b + 1] = (float)(1.0 / (sqrt(var) + 1e-8));
}
}  // namespace

extern "C" {

int kp1_random_permutation(int32_t device, int64_t n, const uint32_t* keys, int64_t* out, void* stream) {
  if (!keys || !out || n <= 0 || n > ((int64_t)1 << 31)) return fail(KP1_ERR_INVALID, "bad argument to kp1_random_permutation");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  int bits = 1;
  while (((int64_t)1 << bits) < n) ++bits;
  PermKeys k;
  for (int r = 0; r < 4; ++r) {
    k.mul[r] = keys[r] | 1u;     // odd: invertible modulo 2^bits
    k.add[r] = keys[4 + r];
  }
  return launch(permutation_kernel, (n + 255) / 256, 256, stream, out, n, bits, k);
}

int kp1_adv_minibatch_stats(int32_t device, const double* sums, int64_t n_minibatches, float* out_stats, void* stream) {
  if (!sums || !out_stats || n_minibatches <= 0) return fail(KP1_ERR_INVALID, "bad argument to kp1_adv_minibatch_stats");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  return launch(adv_minibatch_stats_kernel, (n_minibatches + 63) / 64, 64, stream, sums, n_minibatches, out_stats);
}

int kp1_adv_minibatch_sums(int32_t device, const float* advantages, const int64_t* idx, int64_t total, int64_t minibatch, double* out_sums,
                           void* stream) {
  if (!advantages || !out_sums || total <= 0 || minibatch <= 0) return fail(KP1_ERR_INVALID, "bad argument to kp1_adv_minibatch_sums");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  return launch(adv_minibatch_sums_kernel, (total + minibatch - 1) / minibatch, 256, stream, advantages, idx, total, minibatch, out_sums);
}

int kp1_bootstrap_truncated(int32_t device, float* rewards, const float* terminal_values, const uint8_t* dones, float gamma, int64_t count,
                            void* stream) {
  if (!rewards || !terminal_values || !dones || count <= 0) return fail(KP1_ERR_INVALID, "bad argument to kp1_bootstrap_truncated");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  return launch(bootstrap_kernel, (count + 255) / 256, 256, stream, rewards, terminal_values, dones, gamma, count);
}

int kp1_curriculum_create(int32_t device, double success_rate_threshold, int32_t window_episodes, int32_t min_episodes_per_stage,
                          int32_t max_stage_index, int32_t initial_stage_index, kp1_curriculum_state** out_dev) {
  return kp1_curriculum_create_population(device, 1, success_rate_threshold, window_episodes, min_episodes_per_stage, max_stage_index,
                                          &initial_stage_index, out_dev);
}
int kp1_curriculum_create_population(int32_t device, int32_t n_replicas, double success_rate_threshold, int32_t window_episodes,
                                     int32_t min_episodes_per_stage, int32_t max_stage_index, const int32_t* initial_stages,
                                     kp1_curriculum_state** out_dev) {
  if (!out_dev || !initial_stages) return fail(KP1_ERR_INVALID, "NULL argument");
  if (n_replicas < 1 || n_replicas > KP1_CURRICULUM_MAX_REPLICAS) return fail(KP1_ERR_INVALID, "n_replicas must be in [1, KP1_CURRICULUM_MAX_REPLICAS]");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  std::vector<kp1_curriculum_state> h((size_t)n_replicas);
  for (int k = 0; k < n_replicas; ++k) {
    kp1_curriculum_state& s = h[(size_t)k];
    std::memset(&s, 0, sizeof s);
    s.success_rate_threshold = success_rate_threshold;
    s.window_episodes = window_episodes < 1 ? 1 : window_episodes;  // callbacks.py:45-47 max(..., 1)
    if (s.window_episodes > KP1_CURRICULUM_MAX_WINDOW) return fail(KP1_ERR_INVALID, "window_episodes exceeds KP1_CURRICULUM_MAX_WINDOW");
    s.min_episodes_per_stage = min_episodes_per_stage < 1 ? 1 : min_episodes_per_stage;
    s.max_stage_index = max_stage_index < 0 ? 0 : max_stage_index;
    int init = initial_stages[k] < s.max_stage_index ? initial_stages[k] : s.max_stage_index;
    s.stage_index = init < 0 ? 0 : init;  // callbacks.py:48
  }
  kp1_curriculum_state* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, sizeof(kp1_curriculum_state) * h.size()));
  struct Unowned {   // frees the trackers unless they reached the caller
    void* p;
    ~Unowned() { (void)hipFree(p); }
  } unowned = {d};
  HIP_TRY(hipMemcpy(d, h.data(), sizeof(kp1_curriculum_state) * h.size(), hipMemcpyHostToDevice));
  *out_dev = d;
  unowned.p = nullptr;
  return KP1_OK;
}
int kp1_curriculum_destroy(int32_t device, kp1_curriculum_state* st_dev) {
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  HIP_TRY(hipFree(st_dev));
  return KP1_OK;
}
int kp1_curriculum_observe(int32_t device, kp1_curriculum_state* st_dev, const uint8_t* dones, int32_t n, int32_t steps_per_call, void* stream) {
  if (!st_dev || !dones || n <= 0) return fail(KP1_ERR_INVALID, "bad argument to kp1_curriculum_observe");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  return launch(curriculum_kernel, 1, 64, stream, st_dev, dones, n, steps_per_call);
}
int kp1_curriculum_observe_chunk(int32_t device, kp1_curriculum_state* st_dev, const uint8_t* dones, int32_t n_local, int32_t chunk_steps,
                                 int32_t world, void* stream) {
  if (!st_dev || !dones || n_local <= 0 || chunk_steps <= 0 || world <= 0) return fail(KP1_ERR_INVALID, "bad argument to kp1_curriculum_observe_chunk");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  return launch(curriculum_chunk_kernel, 1, 64, stream, st_dev, dones, n_local, chunk_steps, world, n_local * world);
}
int kp1_curriculum_observe_population(int32_t device, kp1_curriculum_state* states_dev, const uint8_t* dones, int32_t n_per_replica,
                                      int32_t n_replicas, int32_t steps_per_call, void* stream) {
  if (!states_dev || !dones || n_per_replica <= 0 || n_replicas < 1 || n_replicas > KP1_CURRICULUM_MAX_REPLICAS)
    return fail(KP1_ERR_INVALID, "bad argument to kp1_curriculum_observe_population");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  return launch(curriculum_population_kernel, n_replicas, 64, stream, states_dev, dones, n_per_replica, steps_per_call);
}
int kp1_curriculum_read_replica(int32_t device, const kp1_curriculum_state* states_dev, int32_t n_replicas, int32_t k, kp1_curriculum_state* out_host,
                                void* stream) {
  if (!states_dev || !out_host) return fail(KP1_ERR_INVALID, "NULL argument");
  if (k < 0 || k >= n_replicas) return fail(KP1_ERR_INVALID, "replica index out of range");
  return kp1_curriculum_read(device, states_dev + k, out_host, stream);
}
int kp1_curriculum_read(int32_t device, const kp1_curriculum_state* st_dev, kp1_curriculum_state* out_host, void* stream) {
  if (!st_dev || !out_host) return fail(KP1_ERR_INVALID, "NULL argument");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  HIP_TRY(hipMemcpyAsync(out_host, st_dev, sizeof *out_host, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return KP1_OK;
}

}  // extern "C"

// ---- training monitor (include/kp1_ppo.h: kp1_monitor_*, kp1_explained_variance) ---------------------------------------------------------
// SB3's Monitor + ep_info_buffer on the device.  An observe call is two launches:
//   monitor_scan_kernel   one lane per env column, coalesced across a row like the GAE scan: walks t forward with the env's carry in
//                         registers and leaves (return, length) at every position where an episode ends, in a [max_steps][K N] scratch;
//   monitor_rank_kernel   one workgroup per replica: counts the ends of every row (ballots), prefix-sums the row counts in LDS, and gives the
//                         episode at (t, env) the rank (ends of earlier rows) + (ends before it in its row), which is its place in the
//                         (t, env) order; entry j of the call lands in ring slot (head + len + j) mod window, and only the newest `window`
//                         entries are written, so every slot has one writer.
// Nothing waits on another workgroup, every loop is bounded by T, N or the window, and the only arithmetic on a return is the scan's
// sequential double add.
struct kp1_monitor {
  int device, K, N, window, max_steps;
  kp1_monitor_state* states;   // [K]
  double* carry_ret;           // [K N]
  int32_t* carry_len;          // [K N]
  double* ep_ret;              // [max_steps][K N], defined where an episode ended in the last observe call
  int32_t* ep_len;
};

namespace {

__global__ void __launch_bounds__(64) monitor_scan_kernel(const float* __restrict__ rewards, const uint8_t* __restrict__ dones,
                                                          double* __restrict__ carry_ret, int32_t* __restrict__ carry_len,
                                                          double* __restrict__ ep_ret, int32_t* __restrict__ ep_len, int T, int KN) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= KN) return;
  double ret = carry_ret[i];
  int len = carry_len[i];
#pragma unroll 4
  for (int t = 0; t < T; ++t) {
    const int64_t p = (int64_t)t * KN + i;
    ret += (double)rewards[p];
    len += 1;
    if (dones[p] & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) {
      ep_ret[p] = ret;
      ep_len[p] = len;
      ret = 0.0;
      len = 0;
    }
  }
  carry_ret[i] = ret;
  carry_len[i] = len;
}

constexpr int MON_THREADS = 1024, MON_WAVES = MON_THREADS / 64;

__global__ void __launch_bounds__(MON_THREADS) monitor_rank_kernel(kp1_monitor_state* __restrict__ states, const uint8_t* __restrict__ dones,
                                                                   const double* __restrict__ ep_ret, const int32_t* __restrict__ ep_len, int T,
                                                                   int N, int KN) {
  __shared__ int row_off[KP1_MONITOR_MAX_STEPS + 1];   // ends per row, then their exclusive prefix; [T] = all ends of the call
  __shared__ int wave_succ[MON_WAVES];
  __shared__ int hdr[3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t col0 = (int64_t)blockIdx.x * N;
  kp1_monitor_state* __restrict__ st = states + blockIdx.x;
  if (threadIdx.x == 0) {
    hdr[0] = st->window;
    hdr[1] = st->ring_len;
    hdr[2] = st->ring_head;
  }
  // ends (and successes among them) of every row; wave w takes rows w, w + MON_WAVES, ...
  int succ = 0;
  for (int t = wave; t < T; t += MON_WAVES) {
    const uint8_t* __restrict__ row = dones + (int64_t)t * KN + col0;
    int cnt = 0;
    for (int base = 0; base < N; base += 64) {
      const int c = base + lane;
      const uint8_t b = c < N ? row[c] : (uint8_t)0;
      const bool end = (b & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) != 0;
      cnt += __popcll(__ballot(end));
      succ += __popcll(__ballot(end && (b & KP1_DONE_SUCCESS)));
    }
    if (lane == 0) row_off[t] = cnt;
  }
  if (lane == 0) wave_succ[wave] = succ;
  __syncthreads();
  if (wave == 0) {
    int running = 0;
    for (int base = 0; base < T; base += 64) {
      const int t = base + lane;
      const int v = t < T ? row_off[t] : 0;
      int inc = v;
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
      }
      if (t < T) row_off[t] = running + inc - v;
      running += __shfl(inc, 63);
    }
    if (lane == 0) row_off[T] = running;
  }
  __syncthreads();
  const int E = row_off[T];
  if (E == 0) return;                                    // no episode ended: the state keeps every byte
  const int W = hdr[0], len0 = hdr[1], head0 = hdr[2];
  const int skip = E > W ? E - W : 0;                    // older entries of the call would be overwritten by its newer ones
  const unsigned first_slot = (unsigned)(head0 + len0);
  for (int t = wave; t < T; t += MON_WAVES) {
    const int off = row_off[t], cnt = row_off[t + 1] - off;
    if (cnt == 0 || off + cnt <= skip) continue;         // wave-uniform
    const int64_t p0 = (int64_t)t * KN + col0;
    int running = off;
    for (int base = 0; base < N; base += 64) {
      const int c = base + lane;
      const uint8_t b = c < N ? dones[p0 + c] : (uint8_t)0;
      const bool end = (b & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) != 0;
      const unsigned long long m = __ballot(end);
      const int rank = running + __popcll(m & ((1ull << lane) - 1ull));
      if (end && rank >= skip) {
        const unsigned slot = (first_slot + (unsigned)rank) % (unsigned)W;
        st->ring_return[slot] = ep_ret[p0 + c];
        st->ring_length[slot] = ep_len[p0 + c];
        st->ring_success[slot] = (b & KP1_DONE_SUCCESS) ? (uint8_t)1 : (uint8_t)0;
      }
      running += __popcll(m);
    }
  }
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < MON_WAVES; ++w) s += wave_succ[w];
    const long long filled = (long long)len0 + E;
    if (filled > W) {
      st->ring_head = (int)(((long long)head0 + (filled - W)) % W);
      st->ring_len = W;
    } else {
      st->ring_len = (int)filled;
    }
    st->total_episodes += E;
    st->total_successes += s;
  }
}

// One workgroup per replica; thread j takes elements j, j + 1024, ... of the replica's T * N (element e = row e / N, column e % N), then a
// fixed LDS tree: the same sums in the same order on every run.  Shifting by the replica's first element keeps the single-pass form
// well conditioned (and makes a constant buffer's variance exactly 0).
__global__ void __launch_bounds__(1024) explained_variance_kernel(const float* __restrict__ values, const float* __restrict__ returns, int T, int KN,
                                                                  int N, double* __restrict__ out) {
  __shared__ double sums[4][1024];
  const int total = T * N;
  const int64_t col0 = (int64_t)blockIdx.x * N;
  const double y0 = (double)returns[col0], d0 = y0 - (double)values[col0];
  double sy = 0.0, syy = 0.0, sd = 0.0, sdd = 0.0;
  for (int e = threadIdx.x; e < total; e += 1024) {
    const int t = e / N, c = e - t * N;
    const int64_t p = (int64_t)t * KN + col0 + c;
    const double y = (double)returns[p];
    const double ys = y - y0, ds = (y - (double)values[p]) - d0;
    sy += ys;
    syy += ys * ys;
    sd += ds;
    sdd += ds * ds;
  }
  sums[0][threadIdx.x] = sy;
  sums[1][threadIdx.x] = syy;
  sums[2][threadIdx.x] = sd;
  sums[3][threadIdx.x] = sdd;
  __syncthreads();
  for (int k = 512; k > 0; k >>= 1) {
    if (threadIdx.x < k)
#pragma unroll
      for (int q = 0; q < 4; ++q) sums[q][threadIdx.x] += sums[q][threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double n = (double)total;
    const double var_y = (sums[1][0] - sums[0][0] * sums[0][0] / n) / n, var_d = (sums[3][0] - sums[2][0] * sums[2][0] / n) / n;
    out[2 * blockIdx.x] = var_y < 0.0 ? 0.0 : var_y;
    out[2 * blockIdx.x + 1] = var_d < 0.0 ? 0.0 : var_d;
  }
}

void monitor_free(kp1_monitor* m) {
  (void)hipFree(m->states);
  (void)hipFree(m->carry_ret);
  (void)hipFree(m->carry_len);
  (void)hipFree(m->ep_ret);
  (void)hipFree(m->ep_len);
  delete m;
}

}  // namespace

extern "C" {

int kp1_monitor_create(int32_t device, int32_t n_replicas, int32_t n_per_replica, int32_t window, int32_t max_steps, kp1_monitor** out) {
  if (!out) return fail(KP1_ERR_INVALID, "kp1_monitor_create: NULL argument");
  if (n_replicas < 1 || n_replicas > KP1_CURRICULUM_MAX_REPLICAS)
    return fail(KP1_ERR_INVALID, "kp1_monitor_create: n_replicas must be in [1, KP1_CURRICULUM_MAX_REPLICAS]");
  if (n_per_replica < 1) return fail(KP1_ERR_INVALID, "kp1_monitor_create: n_per_replica must be at least 1");
  if (window < 1 || window > KP1_MONITOR_MAX_WINDOW) return fail(KP1_ERR_INVALID, "kp1_monitor_create: window must be in [1, KP1_MONITOR_MAX_WINDOW]");
  if (max_steps < 1 || max_steps > KP1_MONITOR_MAX_STEPS) return fail(KP1_ERR_INVALID, "kp1_monitor_create: max_steps must be in [1, KP1_MONITOR_MAX_STEPS]");
  const int64_t kn = (int64_t)n_replicas * n_per_replica;
  if (kn * max_steps >= ((int64_t)1 << 31)) return fail(KP1_ERR_INVALID, "kp1_monitor_create: max_steps * n_replicas * n_per_replica must stay below 2^31");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  kp1_monitor* m = new kp1_monitor();
  m->device = device; m->K = n_replicas; m->N = n_per_replica; m->window = window; m->max_steps = max_steps;
  m->states = nullptr; m->carry_ret = nullptr; m->carry_len = nullptr; m->ep_ret = nullptr; m->ep_len = nullptr;
  std::vector<kp1_monitor_state> h((size_t)n_replicas);
  std::memset(h.data(), 0, sizeof(kp1_monitor_state) * h.size());
  for (auto& s : h) s.window = window;
  hipError_t e = hipMalloc((void**)&m->states, sizeof(kp1_monitor_state) * h.size());
  if (e == hipSuccess) e = hipMalloc((void**)&m->carry_ret, sizeof(double) * (size_t)kn);
  if (e == hipSuccess) e = hipMalloc((void**)&m->carry_len, sizeof(int32_t) * (size_t)kn);
  if (e == hipSuccess) e = hipMalloc((void**)&m->ep_ret, sizeof(double) * (size_t)(kn * max_steps));
  if (e == hipSuccess) e = hipMalloc((void**)&m->ep_len, sizeof(int32_t) * (size_t)(kn * max_steps));
  if (e == hipSuccess) e = hipMemcpy(m->states, h.data(), sizeof(kp1_monitor_state) * h.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(m->carry_ret, 0, sizeof(double) * (size_t)kn);
  if (e == hipSuccess) e = hipMemset(m->carry_len, 0, sizeof(int32_t) * (size_t)kn);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    monitor_free(m);
    return fail(kp1::status_of(e), std::string("kp1_monitor_create: ") + hipGetErrorString(e));
  }
  *out = m;
  return KP1_OK;
}

int kp1_monitor_destroy(kp1_monitor* mon) {
  if (!mon) return fail(KP1_ERR_INVALID, "kp1_monitor_destroy: NULL argument");
  int rc = use_device(mon->device);
  if (rc != KP1_OK) return rc;
  monitor_free(mon);
  return KP1_OK;
}

int kp1_monitor_observe(kp1_monitor* mon, const float* rewards, const uint8_t* dones, int32_t T, void* stream) {
  if (!mon || !rewards || !dones) return fail(KP1_ERR_INVALID, "kp1_monitor_observe: NULL argument");
  if (T < 1 || T > mon->max_steps) return fail(KP1_ERR_INVALID, "kp1_monitor_observe: T must be in [1, max_steps of the handle]");
  int rc = use_device(mon->device);
  if (rc != KP1_OK) return rc;
  const int KN = mon->K * mon->N;
  rc = launch(monitor_scan_kernel, (KN + 63) / 64, 64, stream, rewards, dones, mon->carry_ret, mon->carry_len, mon->ep_ret, mon->ep_len, T, KN);
  return rc != KP1_OK ? rc : launch(monitor_rank_kernel, mon->K, MON_THREADS, stream, mon->states, dones, mon->ep_ret, mon->ep_len, T, mon->N, KN);
}

int kp1_monitor_reset_carry(kp1_monitor* mon, void* stream) {
  if (!mon) return fail(KP1_ERR_INVALID, "kp1_monitor_reset_carry: NULL argument");
  int rc = use_device(mon->device);
  if (rc != KP1_OK) return rc;
  const size_t kn = (size_t)mon->K * (size_t)mon->N;
  HIP_TRY(hipMemsetAsync(mon->carry_ret, 0, sizeof(double) * kn, (hipStream_t)stream));
  HIP_TRY(hipMemsetAsync(mon->carry_len, 0, sizeof(int32_t) * kn, (hipStream_t)stream));
  return KP1_OK;
}

int kp1_monitor_read(kp1_monitor* mon, int32_t replica, kp1_monitor_state* out_host, void* stream) {
  if (!mon || !out_host) return fail(KP1_ERR_INVALID, "kp1_monitor_read: NULL argument");
  if (replica < 0 || replica >= mon->K) return fail(KP1_ERR_INVALID, "kp1_monitor_read: replica index out of range");
  int rc = use_device(mon->device);
  if (rc != KP1_OK) return rc;
  HIP_TRY(hipMemcpyAsync(out_host, mon->states + replica, sizeof *out_host, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return KP1_OK;
}

int kp1_explained_variance(int32_t device, const float* values, const float* returns, int32_t T, int32_t n_total, int32_t n_per_replica,
                           double* out, void* stream) {
  if (!values || !returns || !out) return fail(KP1_ERR_INVALID, "kp1_explained_variance: NULL argument");
  if (T < 1 || n_total < 1 || n_per_replica < 1 || n_total % n_per_replica != 0)
    return fail(KP1_ERR_INVALID, "kp1_explained_variance: T and n_total must be positive and n_total a multiple of n_per_replica");
  if ((int64_t)T * n_total >= ((int64_t)1 << 31)) return fail(KP1_ERR_INVALID, "kp1_explained_variance: T * n_total must stay below 2^31");
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  return launch(explained_variance_kernel, n_total / n_per_replica, 1024, stream, values, returns, T, n_total, n_per_replica, out);
}

}  // extern "C"
