// kp1_mlp_tile.inc -- one PPO minibatch row tile through the whole activation chain in ONE workgroup (H = 256).
// Included by kp1_mlp.hip inside its anonymous namespace (uses Packed, kp_tanh, f32x4, f32x16, KP1_TR).
//
// The layer-by-layer path (gemm_nt x3 + head_train) is synchronised across the chip: every workgroup loads at the same
// time (HBM-bound, MFMA idle), computes at the same time (HBM idle) and stores at the same time; the tools/nt_timeline.py
// trace of the 28 us layer-2 kernel shows 3.2 us prologue + 18 us MFMA loop + 3.7 us epilogue.  Here a workgroup owns a
// tile of minibatch rows of one net and carries them from the observation to dZ1 without leaving the CU:
//
//   X[BM x 64] --G1--> h1 = tanh(X W1^T + b1) --G2--> h2 = tanh(h1 W2^T + b2) --heads--> mean | value, PPO loss terms,
//   dOut --> dZ2 = (dOut W3)(1 - h2^2) --G3--> dZ1 = (dZ2 W2)(1 - h1^2)
//
// X / h1 / dZ2 / dZ1 tiles are also written to HBM (fire-and-forget stores that drain under the next GEMM) because the
// weight-gradient GEMMs (dW2 = dZ2^T h1, dW1 = dZ1^T X) reduce over the whole minibatch; h2 never leaves LDS.  They are
// written "k8-fragment major" (frag8_at below): [row/8][col/32][lane = col%32 + 32*((row%8)/4)][row%4], the float4 a lane
// of gemm_tn_split_kernel feeds to four consecutive MFMAs as A or B operand, so that kernel needs no LDS staging either.
// That order is also the order a lane holds a 32x32 MFMA accumulator block in (elements 4g .. 4g+3 = rows 8g + 4*(lane/32) .. +3
// of column lane%32), so h1 and dZ1 leave straight from the accumulator registers as coalesced 1 KB wave stores.
// The policy loss needs only the policy net's outputs and the value loss only the value net's, so the two nets are
// independent workgroups (grid.z) exactly as in the layer-wise kernels.
//
// Operands.  A (activations, produced in the kernel) lives in LDS: bufA[BM][260] h1, bufB[BM][260] X -> h2 -> dZ2.
// B (weights) never touches LDS: the packed "fragment-major" copies (Packed::w1f / w2f / w2tf) hold, for every 32-deep
// k stage, MFMA column block and k group, the 64 lanes' float4 B operands contiguously, so one global_load_dwordx4 per
// (column block, k group) is a perfectly coalesced 1 KB wave load straight into the registers the MFMAs read.  A wave
// streams only the weight columns it owns: there is NO barrier inside a GEMM, waves drift apart freely, and the
// stream runs two stages ahead ACROSS the three GEMMs (18 stages, register ring of 3).
//
// Geometry: BM = 32 rows, 4 waves x 2 column blocks, 78.6 KB LDS -> TWO workgroups per CU, so one tile's epilogue / head phase / load
// latency hides under the other tile's MFMAs; training holds the second workgroup of a CU back by 11 us (12 in rounds 1-2) so the two
// do not run their phases in lockstep.  Every weight float4 serves 32 rows: 302 MB pulled from L2 per 8192-row launch (the kernel with
// the MFMAs removed still takes 29.7 of its 51.2 us, profiles/r02_ab_tile32_decomposition.log).  64-row training tiles (one 8-wave
// workgroup per CU) and 8 waves per 32-row tile were measured slower and removed (DESIGN.md 4.1, 4.7).
//
// Every per-tile gradient partial (head weights, biases, log_std, loss sums) is written with plain stores into the same
// hpart / bslab layout head_train_kernel and the dtanh epilogue use, one slot per 32-row tile;
// sums inside the workgroup use shuffles / LDS in a fixed order (no float atomics anywhere => bitwise reproducible).

// what the evaluation forms of the tile (ENV = 3 / 4) need beyond the rollout forms: kp1_eval_accumulate's buffers and step arguments
struct FusedEvalArgs {
  kp1_eval_buffers b;
  int step, confirm, track_ready;
  int last_step;                      // ENV = 5 / 6 (kp1_eval_episodes): env steps step .. last_step in this launch
  double thr_pos, thr_ori, thr_act, thr_dq;
};

struct FusedArgs {
  const float* obs; int64_t obs_stride; int Kreal;   // [rows][obs_stride]; columns >= Kreal read as 0
  int inp;                                            // padded observation width the weights were packed for (64 or 128): picks K1S
  const int64_t* idx; int n;                          // minibatch row gather (or NULL), rows in this minibatch
  Packed k;
  const float* actions; const float* old_logp; const float* adv; const float* ret;
  const double* adv_partials; int n_adv_partials; const float* adv_stats; float adv_mean, adv_inv_std; int adv_mode;
  float clip_range, vf_coef, inv_count;
  float* h1; float* dz2; float* dz1; int64_t act_stride;  // [2][max_batch x 256], k8-fragment major
  float* xf;                                               // gathered observations [max_batch x inp], k8-fragment major
  float* bslab;                                       // db1 partials [32-row slot][2][256]
  float* hpart; int hpart_stride;                     // head partials [32-row slot][10*256 + 32] (layout: HeadArgs::hpart)
  // inference (TRAIN = false: policy.forward of a rollout step / evaluator): any output may be NULL
  const float* noise; float* mean; float* value; float* action; float* clipped; float* log_prob;
  int net_base;                                       // grid.z == 1 launches: which net (0 policy, 1 value) the workgroups run
  int stagger_ticks, n_cus;                           // 32-row training tiles: the second workgroup of every CU starts this many 10 ns ticks late
  StepArgs<float> env;                                // ENV != 0 (kp1_mlp_forward_env_step): row m of the tile IS env m, stepped in this launch
  FusedEvalArgs ev;                                   // ENV = 3 / 4 (kp1_eval_step): the evaluator's bookkeeping of the env step this launch makes
  // [r3, experiment KP1_MLP_OPT_BF16X3_WGRAD] when non-NULL the tile ALSO leaves X / h1 / dZ2 / dZ1 as three bf16 planes (x = hi + mid + lo to 24 bits)
  // in "k16-fragment-major" order for the bf16-MFMA weight-gradient kernel: [plane][net][row/16][col/32][lane][8 bf16], sp_plane elements per plane
  unsigned short* sp_h1; unsigned short* sp_dz2; unsigned short* sp_dz1; unsigned short* sp_xf; int64_t sp_plane, sp_plane_x;
};

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// x = hi + mid + lo with each piece a bf16 (8 significand bits): 24 bits together, the product terms the bf16x3 GEMM keeps reach 2^-24 relative
struct Split3 { bf16x8 hi, mid, lo; };
__device__ __forceinline__ Split3 split3(const float* v) {
  Split3 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 h = (__bf16)v[j];
    const float r1 = v[j] - (float)h;
    const __bf16 m = (__bf16)r1;
    const float r2 = r1 - (float)m;
    o.hi[j] = h;
    o.mid[j] = m;
    o.lo[j] = (__bf16)r2;
  }
  return o;
}
// fragment fi (16 rows) x column block cb of a [rows][ncb * 32] matrix of one net: where a lane's 8 bf16 go.  Element j of lane half h is row
// 16 fi + 8 (j >> 2) + 4 h + (j & 3): the order a lane holds the rows of a 32 x 32 accumulator block in (registers 8 f .. 8 f + 7), and -- k order
// inside an MFMA being free as long as both operands share it -- the order BOTH operands of the weight-gradient GEMM are stored in.
__device__ __forceinline__ void store_split3(unsigned short* __restrict__ base, int64_t plane, int64_t fi, int ncb, int cb, int lane, const Split3& s) {
  const int64_t at = ((fi * ncb + cb) * 64 + lane) * 8;
  *reinterpret_cast<bf16x8*>(base + at) = s.hi;
  *reinterpret_cast<bf16x8*>(base + plane + at) = s.mid;
  *reinterpret_cast<bf16x8*>(base + 2 * plane + at) = s.lo;
}

// element (row b, column col) of a [rows][C] activation matrix in k8-fragment-major order
__host__ __device__ inline int64_t frag8_at(int64_t b, int64_t col, int64_t C) {
  return ((b >> 3) * (C >> 5) + (col >> 5)) * 256 + ((col & 31) + 32 * ((b & 7) >> 2)) * 4 + (b & 3);
}

// The weight-fragment loads are sc1 buffer loads.  The weight stream has no reuse inside a CU (every wave streams its own columns once per
// tile), and pulled through the CU's L1 it evicts what does (observation rows, loss inputs): sc1 / sc0 loads -- served by the L2, not
// allocated in the L1 -- take the training tile from 48.2 to 47.4 us and the rollout tile along with it; nt is 2 us SLOWER
// (profiles/r03_ab_tile_weight_load_policy.log).
__device__ __forceinline__ f32x4 fu_wload(const char* __restrict__ base, unsigned off) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), 0, 0x7fffffff, 0x00020000);
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, AUX_SC1));
}
constexpr int FU_HP = 256, FU_BKS = 32, FU_AP = FU_HP + 4;
constexpr int FU_STAGE = FU_HP * FU_BKS;  // floats of one 32-deep weight stage of one net
constexpr int FU_BM = 32, FU_NW = 4, FU_CB = 2, FU_NTH = 64 * FU_NW;   // rows, waves, 32-column blocks per wave, threads
// dot partials [4 k-quarters][BM][8], dOut [BM][8], per-wave sums [NW][24], misc [64]
constexpr int FU_SCRATCH = 4 * FU_BM * 8 + FU_BM * 8 + FU_NW * 24 + 64;
constexpr int FU_LDS_FLOATS = 2 * FU_BM * FU_AP + HEADS * FU_HP + FU_SCRATCH;
static_assert(FU_LDS_FLOATS * 4 * 2 <= 160 * 1024, "the two training tiles of one CU must fit its LDS");

// TRAIN = false stops after the heads: layer 1 + layer 2 + heads + Gaussian sampling in one launch (replaces two gemm_nt
// launches and head_infer_kernel in the rollout), nothing but the requested outputs is written.
// K1S = 32-deep stages of layer 1: 2 (56-float observation padded to 64) or 4 (80-float route observation padded to 128).
// ENV (inference only) = 1 / 2: the rollout step in ONE launch (approach / dock mode).  The policy workgroup of a tile, once its 32 rows' actions are sampled, hands
// the clipped actions to one lane per row through LDS and that lane runs the whole env step of its env (step_env_lane of kp1_env_step.inc:
// approach / dock mode) -- the action never travels through HBM and the step needs no launch of its own (rollout: 3 -> 2 launches per env
// step).  Such a kernel carries the env step's register footprint (one workgroup per CU: the rollout has one tile per CU anyway).
// ENV = 3 / 4: the deterministic evaluation step in ONE launch (kp1_eval_step for hidden 256; approach / dock mode).  Same forward, policy net
// only (grid.z = 1, net_base 0, noise NULL: every instruction up to the head sum v is the one mlp_tile_kernel<false, 2> issues, so v is the
// mean kp1_mlp_forward writes, bit for bit).  The tail hands clip(v, -1, 1) to the row's lane, which takes its fp64 norm (es_action_norm),
// steps the env without auto-reset and does the evaluator's bookkeeping of that step (eval_account_step) on the fields it has just stored;
// one ballot + one atomicAdd per workgroup counts the episodes still alive.  No action, mean, value or log-prob goes to HBM.
// In place: a.obs is read only by the x-tile load of the prologue (before the first barrier; rows past n re-read row n - 1, a row of the
// same last tile) and observations are written only by store_obs_tile at the very end, each workgroup its own rows, and no value-net
// plane reads them in another workgroup -- a.env.obs == a.obs is legal, and is how kp1_eval_step launches it.
// ENV = 5 / 6: the whole-episode evaluation (kp1_eval_episodes; approach / dock mode) -- the ENV = 3 / 4 form with its body inside a loop over
// env steps a.ev.step .. a.ev.last_step, written as `do { ... } while (EPISODE && ...)` so that the loop does not exist in any other
// instantiation.  Nothing crosses a tile in the evaluator (frozen policy, no auto-reset, no tracker, no RNG, every kp1_eval_buffers entry of
// episode i written by the lane of env i): a workgroup carries its 32 rows through all steps alone, leaves when its last episode has ended
// (or at once when none is alive at entry, nothing written), and adds its alive count to n_alive once.  The loop is bounded by the step span.
//   * A row is stepped only while its episode is alive.  A finished row's observation stays what its last step left: ENV = 5 re-reads it
//     and stores the whole tile, ENV = 6 stores the stepped rows only (ES_EPISODE_REREADS / store_obs_rows; eval_step_kernel's comment in
//     kp1_eval_step.inc says why the two modes differ).
//   * Observation hand-over: wave 0 stores the tile's rows to a.env.obs, all four waves load them as the next iteration's x tile.  The
//     __syncthreads at the bottom of the loop stands between the two: workgroup-scope release (the stores have completed) and acquire.
//     The waves of a workgroup share one CU and its write-through L1, so workgroup scope is sufficient; when the workgroup leaves, the
//     rows are where the ENV = 3 / 4 form leaves them.
//   * The env index and the address of the env config block carry a run-time zero that the loop produces (eval_step_kernel's comment,
//     kp1_eval_step.inc, says why): state addresses and config reads stay inside the iteration, as in the ENV = 3 / 4 form.
//   * The same barrier publishes the alive count wave 0 ballots into one LDS word (misc[2]): the exit is workgroup-uniform.
// SPLIT (training only, [r3 experiment]): the activations leave as three bf16 planes instead of the fp32 k8-fragment copies.  A separate
// instantiation: the exact kernel carries none of its code (as run-time branches in one kernel the extra stores cost the exact path 1 us per launch).
template <bool TRAIN, int K1S, int ENV = 0, bool SPLIT = false>
__global__ void __launch_bounds__(FU_NTH, ENV ? 1 : 2) mlp_tile_kernel(const FusedArgs a) {
  constexpr bool LINE = false;
  constexpr const float* line = nullptr;
#include "kp1_mlp_tile_body.inc"
}

// The training tile of a K = 1 handle whose hyper-parameters live in device memory (kp1_mlp_hparams_store, DESIGN.md section 37):
// mlp_tile_kernel<true, K1S> with clip_range and vf_coef read from `line`, so that a captured graph holds their address and not their
// values.  Same text, same launch shape, same LDS; the bf16x3 experiment (SPLIT) has no line form.  Instantiated by kp1_mlp_line.hip only.
template <int K1S>
__global__ void __launch_bounds__(FU_NTH, 2) mlp_tile_line_kernel(const FusedArgs a, const float* __restrict__ line) {
  constexpr bool TRAIN = true, SPLIT = false, LINE = true;
  constexpr int ENV = 0;
#include "kp1_mlp_tile_body.inc"
}
