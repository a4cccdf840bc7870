// kp1_eval_step.inc -- one step of the batched deterministic evaluator in ONE launch (kp1_eval_step): deterministic policy forward of a row
// tile, the fp64 norm of its clipped action, the env step of the tile's envs and the evaluator's per-episode bookkeeping.
// Included by kp1_mlp.hip inside its anonymous namespace after kp1_env_step.inc (uses kp_tanh, head_dot, f32x16, step_env_lane,
// store_obs_tile) and includes the bookkeeping it shares with eval_accumulate_kernel (kp1_eval_account.inc) and the statements it shares with
// the other tile kernels (kp1_x_tile_body.inc, kp1_row_reread_body.inc; DESIGN.md section 28).
//
// The layer-wise widths (hidden 64 / 128, both in the Hp = 128 layout of struct Packed; observation 56 padded to INP = 64), policy net only.
// grid = (row tiles of ES_BM rows, replicas); row m of replica k is env k n + m of the handle.  A workgroup reads only its own observation
// rows, all of them before the first barrier, and writes them after the last: next_obs == obs is legal and is how the host calls it.
//
// Bit-identity with launch_forward_layers + head_infer_kernel (noise = NULL).  gemm_nt_kernel gives every output element the same chain
// whatever its tiling: v_mfma_f32_32x32x2_f32 over ascending 8-deep k groups, inside a group the float4 components x, y, z, w in order, lanes
// 0-31 / 32-63 carrying k and k + 4; then (acc + bias) through kp_tanh.  Each wave here owns one 32 x 32 output block and issues exactly that
// chain (A operand from the LDS tile at the K + 4 pitch, B operand straight from the k-slab-major weights: the float4 a lane needs is
// contiguous there).  The heads are head_dot's sequential fmaf over k plus the bias, then the clamp head_infer_kernel applies.  All k groups
// of layer 1 are issued, zero padding included, as gemm_nt_kernel does.
#include "kp1_eval_account.inc"

constexpr int ES_BM = 32, ES_NTH = 256, ES_HP = 128, ES_INP = 64;
constexpr int ES_XP = ES_INP + 4, ES_HPITCH = ES_HP + 4;     // LDS pitches (K + 4: the conflict-free b128 operand reads of gemm_nt_kernel)
constexpr int ES_X_FLOATS = ES_BM * ES_XP, ES_H_FLOATS = ES_BM * ES_HPITCH;
// [x | h1] (reused as wave 0's observation tile once the heads are done), h2, actions [ES_BM][8]
constexpr int ES_LDS_FLOATS = ES_X_FLOATS + 2 * ES_H_FLOATS + ES_BM * 8;
static_assert(ES_X_FLOATS + ES_H_FLOATS >= OBS_TILE_FLOATS, "the observation tile of store_obs_tile reuses the x and h1 tiles");
static_assert(ES_NTH == ES_BM * HEADS && ES_NTH / 64 * 32 == ES_HP, "thread = (row, head output); wave = one 32-column block of the hidden width");

struct EvalStepArgs {
  StepArgs<float> env;                 // auto_reset = 0; env.obs is read (this step's observations) and written (the next step's)
  kp1_eval_buffers b;
  const float *w1, *b1, *w2, *b2, *w3, *b3;   // policy net of replica 0 (struct Packed, k-slab major); replica r at + r * r_*
  unsigned r_w1, r_w2, r_b, r_w3, r_b3;
  int n;                               // rows (envs) per replica
  int Kreal;                           // observation columns that are read (56: pitch 56; 64: pitch 64, columns 56.. are the stored zeros)
  int step, confirm;
  int track_ready;
  double thr_pos, thr_ori, thr_act, thr_dq;
  int last_step;                       // episode form: env steps step .. last_step in this launch
};

// one 32 x 32 block of tanh(A W^T + bias): A = ES_BM rows at LDS pitch `apitch`, W k-slab major with N = ES_HP rows, columns [32 wave, +32)
template <int KDIM>
__device__ __forceinline__ void es_layer(const float* __restrict__ as, int apitch, const float* __restrict__ W, const float* __restrict__ bias,
                                         float* __restrict__ out, int wave, int lane) {
  constexpr int KG = KDIM / 8;
  const int col = 32 * wave + (lane & 31), khalf = 4 * (lane >> 5);
  // element (n, k) of W sits at (k / 32) N 32 + n 32 + k % 32: the four k of a lane's operand are one float4
  const float* wl = W + col * 32 + khalf;
  f32x4 bw[KG];
#pragma unroll
  for (int kg = 0; kg < KG; ++kg) bw[kg] = *reinterpret_cast<const f32x4*>(wl + (kg >> 2) * (ES_HP * 32) + (kg & 3) * 8);
  const float bv = bias[col];
  const float* al = as + (lane & 31) * apitch + khalf;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
  for (int kg = 0; kg < KG; ++kg) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(al + kg * 8);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bw[kg].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bw[kg].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bw[kg].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bw[kg].w, acc, 0, 0, 0);
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
    out[row * ES_HPITCH + col] = kp_tanh(acc[e] + bv);
  }
}

// |a| of the seven clipped action values in fp64: products and sums in index order, no contraction, so that the torch expression
// (a0*a0 + a1*a1 + ... + a6*a6).sqrt() on the fp64 cast reproduces it bit for bit
__device__ __forceinline__ double es_action_norm(const float* __restrict__ a) {
#pragma clang fp contract(off)
  double s = __dmul_rn((double)a[0], (double)a[0]);
#pragma unroll
  for (int k = 1; k < ACT; ++k) s = __dadd_rn(s, __dmul_rn((double)a[k], (double)a[k]));
  return sqrt(s);
}

// EPISODE (kp1_eval_episodes): the workgroup carries its ES_BM rows through env steps a.step .. a.last_step by itself and leaves when its last
// episode has ended.  Nothing crosses a tile (frozen policy, no auto-reset, no tracker, no RNG; every kp1_eval_buffers entry of episode i is
// written by the lane that steps env i), so there is no synchronisation between workgroups and the loop is bounded by the step span.
//   * A row is stepped only while its episode is alive (flags[0][i]); the step form steps every row for as long as the host launches.  After
//     the call env i has been stepped counters[0][i] - (its count at entry) times and its handle fields, observation row, reward and done
//     are those of its last step.  A tile without a live episode returns before it writes anything.
//   * A finished row's observation must stay what its last step left, and a lane that does not step has no fresh `o`.  Two equivalent
//     ways: the lane re-reads its row into `o` and store_obs_tile stores the whole tile as in the step form, or only the stepped rows are
//     stored (store_obs_rows).  Which one a mode takes (ES_EPISODE_REREADS) is NOT a matter of taste.  The env step's fp32 sums and reward
//     are not contraction-pinned, and what surrounds the step decides how the compiler fuses them: with the re-read the approach forms
//     reproduce the step form bit for bit and the dock forms differ in the last bit of reward / action_l2 in a few rows; with the row
//     store it is the other way round (every instantiation of both kernels, measured by tests/test_eval_episodes_gpu.py, which is the
//     guard: after a compiler change that test says which choice holds).
//   * Observation hand-over: wave 0 stores the tile's rows to a.env.obs and all four waves load them as the next x tile.  Between the two
//     stands the __syncthreads at the bottom of the loop: a workgroup-scope release (wave 0's stores have completed) and acquire around the
//     barrier.  The waves of a workgroup share one CU and its L1, which the stores write through, so workgroup scope is sufficient; the
//     rows are in HBM-backed memory when the workgroup leaves, as after the step form.
//   * The env's index and its config block are loop-invariant.  Left alone, the compiler lifts the ~100 state-plane addresses of env i and
//     the config reads out of the loop, holds them across the forward (hundreds of spilled registers, written before the loop and re-read
//     in it) and, with multiplies of config terms in another block than their adds, contracts the reward arithmetic differently from the
//     step form (the reward's last bit then differs).  So the env index and the config address carry a run-time zero that the loop
//     produces (the sign bit of the tile's alive count): addresses and config reads stay inside the iteration, as in the step form.
//   * go_on: wave 0 ballots the episodes still alive into one LDS word; every thread reads it after the barrier (a workgroup-uniform exit).
// which episode forms keep a finished row's observation by re-reading it (see eval_step_kernel's comment)
template <int MODE> constexpr bool ES_EPISODE_REREADS = MODE == KP1_MODE_APPROACH;

// store_obs_tile for the episode forms that do not: only the rows whose bit is set in `rows` (the lanes that have just stepped, at most 32) are parked
// and stored; every other row of the block keeps what the env's buffer holds.  EVERY lane of the wave must call this.
__device__ __forceinline__ void store_obs_rows(float* obs, int64_t i0, unsigned rows, const float* o, int stride, float* __restrict__ tile) {
  const int lane = (int)(threadIdx.x & 63u);
  if (lane < 32 && ((rows >> lane) & 1u)) {
    float4* row = reinterpret_cast<float4*>(tile + lane * OBS_TILE_PITCH);
#pragma unroll
    for (int k = 0; k < KP1_OBS_DIM / 4; ++k) row[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    row[14] = make_float4(0.f, 0.f, 0.f, 0.f);
    row[15] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float4* dst = reinterpret_cast<float4*>(obs + i0 * stride);
  const int q4 = stride >> 2;                 // float4 per row: 14 or 16
  for (int f = lane; f < 32 * q4; f += 64) {  // rows 0 .. 31 of the block; unset rows (and rows past the tile's last) are skipped
    const int r = f / q4, c = f - r * q4;
    if ((rows >> r) & 1u) dst[f] = *reinterpret_cast<const float4*>(tile + r * OBS_TILE_PITCH + 4 * c);
  }
}

__device__ __forceinline__ StepArgs<float> es_episode_env(const StepArgs<float>& e, unsigned runtime_zero) {
  StepArgs<float> env = e;
  env.cfg = reinterpret_cast<const DevCfg<float>*>(reinterpret_cast<const char*>(e.cfg) + runtime_zero);
  env.st.n = e.st.n + runtime_zero;    // the plane stride: the scalar halves of the state addresses
  return env;
}

template <int MODE, bool POP, bool EPISODE = false>
__global__ void __launch_bounds__(ES_NTH) eval_step_kernel(const EvalStepArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[ES_LDS_FLOATS];
  float* xs = lds;
  float* h1s = xs + ES_X_FLOATS;
  float* h2s = h1s + ES_H_FLOATS;
  float* acts = h2s + ES_H_FLOATS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned rep = POP ? blockIdx.y : 0u;
  const int m0 = blockIdx.x * ES_BM;
  const int64_t env0 = (int64_t)rep * a.n + m0;          // env of the tile's row 0
  const int rows_live = min(ES_BM, a.n - m0);
  const bool live = lane < rows_live;
  // the x-tile load reads what store_obs_tile wrote in the previous iteration: no __restrict__ on it in the episode form
  using ObsPtr = std::conditional_t<EPISODE, const float*, const float* __restrict__>;
  ObsPtr obs = a.env.obs + (int64_t)rep * a.n * a.env.obs_stride;
  bool alive = false;                  // EPISODE: this lane's episode (every wave holds the tile's flags; wave 0 keeps them current)
  if constexpr (EPISODE) {
    alive = live && a.b.flags[env0 + lane] != 0;
    if (!__ballot(alive)) return;      // the same answer in all four waves: nothing has written a flag yet
  }
  int step = a.step, n_alive_tile = 0;
  unsigned runtime_zero = 0;           // EPISODE: see es_episode_env

  do {
  // ---- 1. the tile's observation rows -> LDS (rows past the replica's last and columns >= Kreal read as zero, as gemm_nt_kernel masks them)
  {
    constexpr int X_INP = ES_INP, X_PITCH = ES_XP;
    const int x_n = a.n, x_stride = a.env.obs_stride, x_kreal = a.Kreal;
#include "kp1_x_tile_body.inc"
  }
  __syncthreads();

  // ---- 2. policy net: h1, h2, heads, clamp
  es_layer<ES_INP>(xs, ES_XP, a.w1 + (POP ? rep * a.r_w1 : 0u), a.b1 + (POP ? rep * a.r_b : 0u), h1s, wave, lane);
  __syncthreads();
  es_layer<ES_HP>(h1s, ES_HPITCH, a.w2 + (POP ? rep * a.r_w2 : 0u), a.b2 + (POP ? rep * a.r_b : 0u), h2s, wave, lane);
  __syncthreads();
  {
    const int row = tid >> 3, out = tid & 7;
    float v = 0.f;
    if (out < ACT) {
      v = head_dot(h2s + row * ES_HPITCH, a.w3 + (POP ? rep * a.r_w3 : 0u) + out * ES_HP, ES_HP) + a.b3[(POP ? rep * a.r_b3 : 0u) + out];
      v = fminf(fmaxf(v, -1.f), 1.f);
    }
    acts[row * 8 + out] = v;
  }
  __syncthreads();
  if constexpr (!EPISODE) {
    if (wave != 0) return;
  }

  // ---- 3.-6. lane r of wave 0: action norm, env step, bookkeeping of env env0 + r; then the wave stores the tile's next observations
  if (!EPISODE || wave == 0) {
    float o[KP1_OBS_DIM];
    int alive_after = 0;
    if (EPISODE ? alive : live) {
      const int64_t i = env0 + lane + (EPISODE ? runtime_zero : 0u);
      const double an = es_action_norm(acts + lane * 8);
      if constexpr (EPISODE) step_env_lane<float, MODE, false>(es_episode_env(a.env, runtime_zero), i, acts + lane * 8, o);
      else step_env_lane<float, MODE, false>(a.env, i, acts + lane * 8, o);
      // the fields the step has just stored are read back from the handle by the lane that stored them
      alive_after = eval_account_step<float>(a.env.st.real, (int)a.env.st.n, (int)i, a.b, an, a.env.done[i], step, a.track_ready != 0, a.thr_pos,
                                             a.thr_ori, a.thr_act, a.thr_dq, a.confirm);
    } else if (EPISODE && ES_EPISODE_REREADS<MODE> && live) {
      // a finished (or never started) episode is not stepped: its row of the tile is its current observation
      const f32x4* src = reinterpret_cast<const f32x4*>(obs + (int64_t)(m0 + lane) * a.env.obs_stride);
#include "kp1_row_reread_body.inc"
    }
    const unsigned long long bal = __ballot(alive_after != 0);
    if constexpr (!EPISODE) {
      if (lane == 0 && bal) atomicAdd(a.b.n_alive, __popcll(bal));
    }
    // x and h1 were last read two barriers ago
    if constexpr (EPISODE && !ES_EPISODE_REREADS<MODE>) store_obs_rows(a.env.obs, env0, (unsigned)__ballot(alive), o, a.env.obs_stride, lds);
    else store_obs_tile(a.env.obs, env0, rows_live, o, live, a.env.obs_stride, lds);
    if constexpr (EPISODE) {
      alive = alive_after != 0;
      if (lane == 0) reinterpret_cast<int*>(acts)[0] = __popcll(bal);   // acts: this wave alone read it, and has finished
    }
  }
  if constexpr (EPISODE) {
    __syncthreads();                   // the tile's new observation rows and the alive count, for all four waves
    n_alive_tile = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(acts)[0]);
    runtime_zero = (unsigned)n_alive_tile >> 31;   // a count is never negative
  }
  } while (EPISODE && n_alive_tile != 0 && step++ < a.last_step);
  if constexpr (EPISODE) {
    if (tid == 0 && n_alive_tile) atomicAdd(a.b.n_alive, n_alive_tile);
  }
}
