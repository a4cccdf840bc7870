// kp1_rollout_step.inc -- one rollout step of the layer-wise widths in ONE launch (kp1_mlp_forward_env_step on an Hp = 128 handle): stochastic
// policy forward of a row tile (both nets), Gaussian sampling, and the env step of the tile's envs with its fused auto-reset.
// Included by kp1_mlp.hip inside its anonymous namespace after kp1_eval_step.inc (uses es_layer and the ES_* geometry, head_dot, kp_tanh,
// step_env_lane, store_obs_tile; x tile and sampling tail are the statement files every tile kernel includes, DESIGN.md section 28).
//
// Hidden 64 / 128, both in the Hp = 128 layout of struct Packed; observation 56 at pitch 56 or 64 (INP = 64).
// grid = (row tiles of ES_BM rows, replicas, value ? 2 : 1), 256 threads; row m of replica k is env k n + m of the env handle.  Plane z = 0 runs
// the policy net, samples, and steps the tile's envs from wave 0; plane z = 1 runs the value net and touches nothing of the env.  The value net
// is a z-plane and not four more waves: the lane that steps an env runs the fused reset branch (128-bit PCG64, fp64 samplers) and needs the
// whole unified register budget of a one-wave-per-SIMD workgroup.  The two planes read the same observation rows and write disjoint outputs;
// the step's observations go to next_obs != obs (the entry point refuses next_obs == obs), so plane 1 never reads a row plane 0 has written.
//
// Bit-identity with the launch sequence launch_forward_layers + head_infer_kernel + kp1_step_kernel:
//  * hidden layers, either net: the argument at the top of kp1_eval_step.inc.  gemm_nt_kernel gives every output element the same chain
//    whatever its tiling or its net (blockIdx.z there only moves the base pointers); es_layer issues exactly that chain on the net's weights.
//  * heads: head_infer_kernel computes head `out` of a row as head_dot over the Hp floats of the row's h2 (the policy net's for out 0..6, the
//    value net's for out 7) against row `out` of w3, plus b3[out].  head_dot is a sequential fmaf over k: reading w3 and h2 from LDS or global
//    memory, or the row from one plane or the other, does not change it.  value[row] is that number for out 7, stored unchanged.
//  * sampling tail: head_infer_kernel's expressions, in the one text every one-launch rollout form includes (kp1_sample_tail_body.inc): the
//    action, the log-density term per action lane and 0 for lane 7, then the three __shfl_xor sums over the 8-lane group.  The thread =
//    (row = t / 8, out = t % 8) mapping is head_infer_kernel's, so every shuffle adds the same two partial sums in the same order.  Rows past
//    the replica's last carry lp = 0 there and here and are never stored; a group never mixes rows.
//  * env step: the launch sequence hands kp1_step_kernel clipped = fminf(fmaxf(act, -1.f), 1.f) through global memory; the same value goes to
//    the row's lane through LDS (so a NaN action clips as it does there), and step_env_lane is the body of kp1_step_kernel.
// No float atomics anywhere; every output element has one writer.

struct RolloutStepArgs {
  StepArgs<float> env;                 // auto_reset = 1; env.obs = next_obs (written only)
  const float* obs;                    // this step's observations, [K n][obs_stride]
  int obs_stride;
  const float *w1, *b1, *w2, *b2;      // net 0 of replica 0 (struct Packed, k-slab major); net z at + z * n_*, replica r at + r * r_*
  const float *w3, *b3, *log_std;      // [K][8][Hp], [K][8], [K][8]
  unsigned r_w1, r_w2, r_b, r_w3, r_b3;
  unsigned n_w1, n_w2, n_b;
  const float* noise;                  // [K n][7]
  float* value;                        // [K n] or nullptr (then no z = 1 plane is launched)
  float* action;                       // [K n][7], unclipped
  float* log_prob;                     // [K n] or nullptr
  int n;                               // rows (envs) per replica
  int Kreal;                           // observation columns that are read (56: pitch 56; 64: pitch 64, columns 56.. are the stored zeros)
};

// POP: the env handle is bound to a population (per-replica stages / dock stage records), step_env_lane's POP form.  The weights' replica is
// the grid's y in either form (a K = 1 handle launches y = 1).
template <int MODE, bool POP>
__global__ void __launch_bounds__(ES_NTH) rollout_step_kernel(const RolloutStepArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[ES_LDS_FLOATS];
  float* xs = lds;
  float* h1s = xs + ES_X_FLOATS;
  float* h2s = h1s + ES_H_FLOATS;
  float* acts = h2s + ES_H_FLOATS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned rep = blockIdx.y, net = blockIdx.z;
  const int m0 = blockIdx.x * ES_BM;
  const int64_t env0 = (int64_t)rep * a.n + m0;          // env of the tile's row 0

  // ---- 1. the tile's observation rows -> LDS (rows past the replica's last and columns >= Kreal read as zero, as gemm_nt_kernel masks them)
  {
    constexpr int X_INP = ES_INP, X_PITCH = ES_XP;
    const int x_n = a.n, x_stride = a.obs_stride, x_kreal = a.Kreal;
    const float* __restrict__ obs = a.obs + (int64_t)rep * a.n * a.obs_stride;
#include "kp1_x_tile_body.inc"
  }
  __syncthreads();

  // ---- 2. hidden layers of this plane's net
  es_layer<ES_INP>(xs, ES_XP, a.w1 + rep * a.r_w1 + net * a.n_w1, a.b1 + rep * a.r_b + net * a.n_b, h1s, wave, lane);
  __syncthreads();
  es_layer<ES_HP>(h1s, ES_HPITCH, a.w2 + rep * a.r_w2 + net * a.n_w2, a.b2 + rep * a.r_b + net * a.n_b, h2s, wave, lane);
  __syncthreads();

  const int row = tid >> 3, out = tid & 7;
  const bool ok = m0 + row < a.n;
  const float* __restrict__ w3 = a.w3 + rep * a.r_w3;
  const float* __restrict__ b3 = a.b3 + rep * a.r_b3;

  // ---- z = 1: the value head of the tile's rows
  if (net != 0) {
    if (ok && out == HEADS - 1) a.value[env0 + row] = head_dot(h2s + row * ES_HPITCH, w3 + out * ES_HP, ES_HP) + b3[out];
    return;
  }

  // ---- 3. z = 0: action heads and head_infer_kernel's sampling tail
  {
    constexpr bool TAIL_STORES_CLIPPED = false;
    const RolloutStepArgs fw = a;      // a copy, not a reference: see the fragment's header
    const int64_t tail_off = 0;
    float* const tail_clipped = nullptr;
#include "kp1_sample_tail_body.inc"
  }
  __syncthreads();
  if (wave != 0) return;

  // ---- 4. lane r of wave 0 steps env env0 + r (auto-reset included); then the wave stores the tile's next observations
  const int rows_live = min(ES_BM, a.n - m0);
  const bool live = lane < rows_live;
  float o[KP1_OBS_DIM];
  if (live) step_env_lane<float, MODE, false, POP>(a.env, env0 + lane, acts + lane * 8, o);
  // x and h1 were last read two barriers ago
  store_obs_tile(a.env.obs, env0, rows_live, o, live, a.env.obs_stride, lds);
}
