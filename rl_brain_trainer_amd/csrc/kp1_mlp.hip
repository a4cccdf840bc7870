// kp1_mlp.hip -- actor-critic MLP forward / loss / backward / Adam on gfx950 matrix cores.
//
// Arithmetic: fp32 in, fp32 accumulate (v_mfma_f32_32x32x2_f32: exact f32, 64 FLOP/clk/SIMD = 157 TFLOP/s chip peak).
// The reference trains in fp32 (SB3 on torch defaults), so no reduced-precision operands are used.
//
// GEMM shapes per optimiser step (B = minibatch rows, H = hidden, both nets batched in grid.z):
//   fwd   Z1 = X[B,64] W1p^T      Z2 = H1[B,H] W2^T                         -> gemm_nt  (A row-major, W row-major [N][K])
//   bwd   dZ1 = (dZ2[B,H] W2) * (1 - H1^2)   (uses the packed transpose W2T) -> gemm_nt
//   wgrad dW2 = dZ2^T H1 , dW1 = dZ1^T X      (reduction over B, split-K)     -> gemm_tn
// The 7+1 wide heads, the PPO loss and its gradient run on the vector ALUs in head kernels.
//
// MFMA operand scheme (32x32x2): lane l feeds A[i = l&31][kslot = l>>5] and B[kslot][j = l&31]; C/D element
// (row = (reg&3) + 8*(reg>>2) + 4*(l>>5), col = l&31).  K order inside a tile is free, so each lane reads 4 (NT) or
// 1 (TN) consecutive k per LDS read and both operands use the same k for the same kslot.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

#include "../../include/kp1_ppo.h"
#include "../../include/kp1_route.h"
#include "../../include/kp1_ziggurat_tables.h"
#include "kp1_device.hpp"
#include "kp1_host.hpp"

using kp1::fail;
using namespace kp1;   // kp1_device.hpp: the env arithmetic the rollout kernel steps its tile's envs with

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vector: arrays of it are reliably scalar-replaced (HIP's float4 struct was not)

namespace {

constexpr int ACT = KP1_MLP_ACT, HEADS = 8;  // observation width: ParamLayout::IN (56, or 80 with the route keys), padded to INP (64 / 128)
constexpr float LOG_SQRT_2PI = 0.9189385332046727f;

enum { EPI_BIAS_TANH = 0, EPI_DTANH = 1 };

// Developer timeline (tools/nt_timeline.py builds a private copy of the library with -DKP1_NT_TRACE): thread 0 of every
// workgroup stamps the 100 MHz wall clock at the phase boundaries of gemm_nt_kernel.  Compiled out of the product.
#ifdef KP1_NT_TRACE
constexpr int KP1_TRACE_SLOTS = 16, KP1_TRACE_WGS = 1024;
__device__ unsigned long long kp1_nt_trace_buf[KP1_TRACE_SLOTS * KP1_TRACE_WGS];
#define KP1_TR(slot)                                                                                          \
  if (threadIdx.x == 0) {                                                                                     \
    const int wg_ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);                           \
    if (wg_ < KP1_TRACE_WGS) kp1_nt_trace_buf[wg_ * KP1_TRACE_SLOTS + (slot)] = wall_clock64();               \
  }
// where the workgroup runs: HW_ID (cu_id [11:8], sh_id [12], se_id [15:13]) in the low word, XCC_ID in the high word
#define KP1_TR_HW(slot)                                                                                       \
  if (threadIdx.x == 0) {                                                                                     \
    const int wg_ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);                           \
    if (wg_ < KP1_TRACE_WGS)                                                                                  \
      kp1_nt_trace_buf[wg_ * KP1_TRACE_SLOTS + (slot)] =                                                      \
          (unsigned long long)__builtin_amdgcn_s_getreg(63492) | ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32); \
  }
#else
#define KP1_TR(slot)
#define KP1_TR_HW(slot)
#endif

// Developer check of the shader clock the matrix kernels actually run at (the guide's DVFS item 6: cycles of s_memtime per tick of the 100 MHz
// s_memrealtime, stamped once at the start and once at the end of a workgroup; tools/mfma_clock.py builds with -DKP1_CLK_TRACE).  The stamps go to
// a buffer nothing else reads.  Compiled out of the product.
#ifdef KP1_CLK_TRACE
__device__ unsigned long long kp1_clk_buf[2 * 1024 * 4];   // [kernel: 0 tile, 1 weight gradients][workgroup][cycles at start, ticks, cycles at end, ticks]
#define KP1_CLK(kern, at)                                                                                     \
  if (threadIdx.x == 0) {                                                                                     \
    const int wg_ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);                           \
    if (wg_ < 1024) {                                                                                         \
      kp1_clk_buf[((kern) * 1024 + wg_) * 4 + 2 * (at)] = __builtin_readcyclecounter();                       \
      kp1_clk_buf[((kern) * 1024 + wg_) * 4 + 2 * (at) + 1] = wall_clock64();                                 \
    }                                                                                                         \
  }
#else
#define KP1_CLK(kern, at)
#endif

// Cache policy of the big once-written / once-read streams (the measured optimum): aux bits of the gfx950 buffer instructions,
// 1 = sc0, 2 = nt, 16 = sc1.  sc1 stores are write-through: the line leaves the XCD's L2 when it is written instead of at the kernel's
// end-of-launch write-back, and the consumer (another launch, mostly on another XCD) reads it from HBM / the memory-side cache either way.
//   weight-gradient partial-slab stores: sc1 (write-through: 30.4 -> 29.0 us in situ, profiles/r02_ab_cache_policy.log)
//   weight-gradient activation-fragment loads: sc1, they bypass the CU's L1 (no reuse inside a CU): 25.4 -> 24.4 us in situ, nt 26.5
//     (profiles/r03_ab_tn_load_policy.log)
//   tile-kernel activation stores and finalize-kernel slab loads: plain
constexpr int AUX_SC1 = 16;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// 16-byte sc1 store of `v` at float index `idx` of the (wave-uniform) base pointer
__device__ __forceinline__ void store16_sc1(float* __restrict__ base, int64_t idx, const f32x4 v) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7fffffff, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)(idx * 4), 0, AUX_SC1);
}
// 16-byte sc1 load at base[off] (floats)
__device__ __forceinline__ f32x4 load16_sc1(const float* __restrict__ base, int64_t off) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, 0x7fffffff, 0x00020000);
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)(off * 4), 0, AUX_SC1));
}

// tanh(x) = 2 / (1 + 2^(-2 log2(e) x)) - 1 in FIVE vector instructions (v_mul, v_exp_f32, v_add, v_rcp_f32, v_fma = 28 issue cycles).
// Instruction count matters more here than anywhere else in the kernel: v_mfma_f32_32x32x2_f32 runs on the SIMD's fp32 FMA lanes, so
// vector-ALU work never overlaps with fp32 MFMAs -- not inside a wave (one v_fma between two MFMAs costs its full 4 cycles on top of the
// MFMA's 64) and not across co-resident waves (a VALU-only wave next to an MFMA-only wave finishes in the SUM of both times);
// tools/mfma_valu_mix.hip, profiles/r02_mfma_valu_mix.log.  Every vector instruction of an epilogue is therefore paid in MFMA time, and
// the 64 tanh evaluations per lane were 38 % of the tile kernel's vector instructions in the round-1 form (14 instructions each: odd
// polynomial below |x| = 0.25, exp form above, select, copysign).  Saturates correctly (2^(+big) = inf -> -1, 2^(-big) = 0 -> +1), NaN
// propagates.  Absolute error <= ~1.8e-7 on [-20, 20] with exact exp2 and rcp (the rounding of 1 + t and of the final 2r - 1), i.e. fp32
// epsilon of the result's scale; the RELATIVE error grows as |x| -> 0 (result ~ x +- 1e-7), which a tanh hidden unit's consumers -- dot
// products of 256 such values, and 1 - h^2 in the backward pass -- do not resolve.  Held against fp64 up to |x| ~ 49 and at |x| ~ 1e18 by
// tests/test_trained_regime_gpu.py (through the kernels that use it); DESIGN.md, "Parity on trained-scale policies".
__device__ __forceinline__ float kp_tanh(float x) {
  const float t = __builtin_amdgcn_exp2f(x * -2.8853900817779268f);
  return fmaf(2.0f, __builtin_amdgcn_rcpf(t + 1.0f), -1.0f);
}

struct GemmNT {
  const float* A; int64_t lda; int64_t strideA;       // [M][lda], per-net stride
  const int64_t* gather;                               // optional row indices into A (shared by both nets)
  const float* W; int64_t strideW;                     // k-slab major [K/32][N][32] (struct Packed)
  const float* bias; int64_t strideBias;               // [N]
  float* C; int64_t ldc; int64_t strideC;              // [M][ldc]
  const float* aux; int64_t strideAux;                 // EPI_DTANH: activation H at C's coordinates (ld = ldc)
  float* colsum; int64_t strideColsum;                 // EPI_DTANH: per-row-block column sums of C (bias-gradient partials)
                                                       //   written to colsum[blockIdx.x * 2*strideColsum + z*strideColsum + n]
  int M, N, K, Kreal;                                  // K multiple of 32; A columns >= Kreal read as 0
  // population handles (POP kernels): grid.z = 2 * reps, z = 2 * replica + net; replica r reads / writes at base + r * r_* (elements)
  int reps;
  unsigned r_A, r_gather, r_W, r_bias, r_C, r_aux, r_colsum;
};

// C = epi(A W^T).  One workgroup owns 64 rows x BN columns (BN = 256: the whole hidden width, or 128 for small
// batches) for one net.  The 64 x K block of A is loaded ONCE and stays in LDS; W streams through a double-buffered
// [BN][32] stage, so every stage carries 4096 MFMA cycles per wave (BN = 256) against one L2 round trip, and A is
// never re-read.  4 waves, each 64 columns wide (2 MFMA column blocks) and RB row blocks tall.
// amdgpu_waves_per_eu(1, 2): the 140 KB LDS footprint allows one workgroup (one wave per SIMD) per CU anyway; without
// the hint hipcc spills the prefetch registers to scratch to stay under the 256-register budget of two waves per SIMD.
template <int BN, int EPI, int K, int NTH, int BM, int BKS, bool POP = false>
__global__ void __launch_bounds__(NTH) gemm_nt_kernel(const GemmNT g) {
  constexpr int NW = NTH / 64, LDS_T = BKS + 4, KC = BKS / 4;  // BKS = k depth of one W stage, LDS_T its LDS pitch  // NTH = 512: two waves per SIMD share the MFMA pipe and split the epilogue VALU work
  constexpr int KQ = K / 4, A_LOADS = BM * KQ / NTH;  // float4 per A row / per thread: all issued before any is used
  constexpr int WN = BN / 64, WM = NW / WN;
  constexpr int RB = BM / WM / 32, CB = 2;
  constexpr int W_LOADS = BN * KC / NTH;
  extern __shared__ float lds[];
  constexpr int lda_s = K + 4;               // LDS pitch of the resident A block (bank-conflict-free b128 reads)
  float* As = lds;
  float* Ws0 = lds + BM * lda_s;
  float* Ws1 = Ws0 + BN * LDS_T;

  const int z = POP ? (int)(blockIdx.z & 1u) : (int)blockIdx.z;
  const unsigned rep = POP ? blockIdx.z >> 1 : 0u;   // replica of a population handle (0: single handle)
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const float* __restrict__ A = g.A + (POP ? rep * g.r_A : 0u) + z * g.strideA;
  const float* __restrict__ W = g.W + (POP ? rep * g.r_W : 0u) + z * g.strideW + (int64_t)n0 * 32;  // k-slab major: [K/32][N][32]
  const int64_t* __restrict__ gather = (POP && g.gather) ? g.gather + rep * g.r_gather : g.gather;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave / WN, wc = wave % WN;

  // ---- prologue: W stages 0 and 1 to registers, whole A block to LDS.  W is prefetched TWO stages ahead (register
  // sets rwa / rwb alternate): with one wave per SIMD nothing else hides an L2 round trip, and one 4096-cycle stage
  // of cover was not enough under 256 workgroups streaming the same W.
  constexpr int KT = K / BKS;
  f32x4 rwa[W_LOADS], rwb[W_LOADS];
#define KP1_NT_WLOAD(dst, stage)                                                                        \
  {                                                                                                     \
    const int kk = ((stage) < KT ? (stage) : KT - 1) * BKS;                                              \
    _Pragma("unroll") for (int j = 0; j < W_LOADS; ++j) {                                               \
      const int f = tid + NTH * j;                                                                      \
      dst[j] = *reinterpret_cast<const f32x4*>(W + (int64_t)(kk >> 5) * g.N * 32 + (f / KC) * 32 + (kk & 31) + 4 * (f % KC)); \
    }                                                                                                   \
  }
#define KP1_NT_WSTORE(src, ws)                                                                          \
  _Pragma("unroll") for (int j = 0; j < W_LOADS; ++j) {                                                 \
    const int f = tid + NTH * j;                                                                        \
    *reinterpret_cast<f32x4*>((ws) + (f / KC) * LDS_T + 4 * (f % KC)) = src[j];                            \
  }
  KP1_TR(0)
  KP1_NT_WLOAD(rwa, 0)
  KP1_NT_WLOAD(rwb, 1)
  {
    // branch-free and fully unrolled: (gather indices) -> all A_LOADS row loads in flight -> mask -> LDS
    int64_t arow[A_LOADS];
    f32x4 av[A_LOADS];
#pragma unroll
    for (int j = 0; j < A_LOADS; ++j) {
      const int m = min(m0 + (tid + NTH * j) / KQ, g.M - 1);
      arow[j] = gather ? gather[m] : (int64_t)m;
    }
#pragma unroll
    for (int j = 0; j < A_LOADS; ++j) {
      const int k = 4 * ((tid + NTH * j) % KQ);
      av[j] = *reinterpret_cast<const f32x4*>(A + arow[j] * g.lda + (k < g.Kreal ? k : 0));
    }
#pragma unroll
    for (int j = 0; j < A_LOADS; ++j) {
      const int f = tid + NTH * j, row = f / KQ, k = 4 * (f % KQ);
      const float keep = (m0 + row < g.M && k < g.Kreal) ? 1.f : 0.f;
      *reinterpret_cast<f32x4*>(As + row * lda_s + k) = av[j] * keep;
    }
  }
  KP1_NT_WSTORE(rwa, Ws0)
  __syncthreads();
  KP1_TR(1)

  f32x16 acc[RB][CB];
#pragma unroll
  for (int r = 0; r < RB; ++r)
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[r][c][e] = 0.f;

  const float* as_base = As + (wr * (BM / WM) + (lane & 31)) * lda_s + 4 * (lane >> 5);
#define KP1_NT_COMPUTE(kt_, ws_cur_)                                                                    \
  {                                                                                                     \
    const float* as = as_base + (kt_) * BKS;                                                             \
    const float* ws = (ws_cur_) + (wc * 64 + (lane & 31)) * LDS_T + 4 * (lane >> 5);                      \
    _Pragma("unroll") for (int kg = 0; kg < BKS / 8; ++kg) {                                             \
      float4 a[RB], b[CB];                                                                              \
      _Pragma("unroll") for (int r = 0; r < RB; ++r) a[r] = *reinterpret_cast<const float4*>(as + r * 32 * lda_s + kg * 8); \
      _Pragma("unroll") for (int c = 0; c < CB; ++c) b[c] = *reinterpret_cast<const float4*>(ws + c * 32 * LDS_T + kg * 8);   \
      _Pragma("unroll") for (int r = 0; r < RB; ++r)                                                    \
        _Pragma("unroll") for (int c = 0; c < CB; ++c) {                                                \
          acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r].x, b[c].x, acc[r][c], 0, 0, 0);         \
          acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r].y, b[c].y, acc[r][c], 0, 0, 0);         \
          acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r].z, b[c].z, acc[r][c], 0, 0, 0);         \
          acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r].w, b[c].w, acc[r][c], 0, 0, 0);         \
        }                                                                                               \
    }                                                                                                   \
  }
  // stage kt computes from LDS buffer (kt & 1); registers hold stage kt+1 (written to the other buffer at the end of
  // the stage) while the loads of stage kt+2 are issued at its start.  Unrolled by two so the register sets are static.
  for (int kt = 0; kt < KT; kt += 2) {
    KP1_NT_WLOAD(rwa, kt + 2)          // rwa is free: stage kt already sits in Ws0
    KP1_NT_COMPUTE(kt, Ws0)
    KP1_NT_WSTORE(rwb, Ws1)            // stage kt+1
    __syncthreads();
    KP1_NT_WLOAD(rwb, kt + 3)          // KT is even (K % 64 == 0, checked on the host): no conditional, no spills
    KP1_NT_COMPUTE(kt + 1, Ws1)
    KP1_NT_WSTORE(rwa, Ws0)            // stage kt+2
    __syncthreads();
    KP1_TR(2 + kt / 2)
  }
#undef KP1_NT_WLOAD
#undef KP1_NT_WSTORE
#undef KP1_NT_COMPUTE

  // ---- epilogue: accumulators -> LDS (row-major [64][BN+4], reusing the A/W staging space) -> each thread owns
  // float4 column groups of 16 B, so bias/aux loads and the C stores are fully coalesced dwordx4 (the MFMA register
  // layout would give 64 scalar stores per lane, which are issue-bound with one wave per SIMD).
  constexpr int LDC = BN + 4, CQ = BN / 4, C_ITERS = BM * CQ / NTH;
  float* Cs = lds;
#pragma unroll
  for (int c = 0; c < CB; ++c)
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wr * (BM / WM) + r * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        Cs[row * LDC + wc * 64 + c * 32 + (lane & 31)] = acc[r][c][e];
      }
  __syncthreads();
  KP1_TR(10)
  float* __restrict__ C = g.C + (POP ? rep * g.r_C : 0u) + z * g.strideC;
  const int c4 = tid % CQ;                      // fixed column group per thread
  const int ncol = n0 + 4 * c4;
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if constexpr (EPI == EPI_BIAS_TANH) bias4 = *reinterpret_cast<const f32x4*>(g.bias + (POP ? rep * g.r_bias : 0u) + z * g.strideBias + ncol);
  f32x4 hv[EPI == EPI_DTANH ? C_ITERS : 1];
  if constexpr (EPI == EPI_DTANH) {
#pragma unroll
    for (int j = 0; j < C_ITERS; ++j) {
      const int m = min(m0 + (tid + NTH * j) / CQ, g.M - 1);
      hv[j] = *reinterpret_cast<const f32x4*>(g.aux + (POP ? rep * g.r_aux : 0u) + z * g.strideAux + (int64_t)m * g.ldc + ncol);
    }
  }
  f32x4 csum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < C_ITERS; ++j) {
    const int row = (tid + NTH * j) / CQ;
    const int m = m0 + row;
    f32x4 v = *reinterpret_cast<const f32x4*>(Cs + row * LDC + 4 * c4);
    if constexpr (EPI == EPI_BIAS_TANH) {
      v += bias4;
      v.x = kp_tanh(v.x); v.y = kp_tanh(v.y); v.z = kp_tanh(v.z); v.w = kp_tanh(v.w);
    } else {
      v = v * (1.f - hv[j] * hv[j]);
      if (m < g.M) csum += v;
    }
    if (m < g.M) *reinterpret_cast<f32x4*>(C + (int64_t)m * g.ldc + ncol) = v;
  }
  KP1_TR(11)
  if constexpr (EPI == EPI_DTANH) {
    if (g.colsum) {
      // bias-gradient partial of this row block: threads tid, tid + CQ, ... own the same column group; combine them in
      // LDS (space behind the C tile) and write one row of partials with plain stores (no contended atomics)
      float* red = lds + BM * LDC;
      *reinterpret_cast<f32x4*>(red + (tid / CQ) * BN + 4 * c4) = csum;
      __syncthreads();
      if (tid < BN) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < NTH / CQ; ++k) t += red[k * BN + tid];
        g.colsum[(POP ? rep * g.r_colsum : 0u) + (int64_t)blockIdx.x * 2 * g.strideColsum + z * g.strideColsum + n0 + tid] = t;
      }
    }
  }
}

struct GemmTN {
  const float* D; int64_t ldd; int64_t strideD;     // dZ [B][ldd] : output-feature columns ("M" of the product)
  const float* X; int64_t ldx; int64_t strideX;     // previous activations [B][ldx] : input-feature columns ("N")
  const int64_t* gatherX;                            // optional row gather for X (layer 1 reads the obs buffer)
  float* slab;                                       // partial products [chunk][net][Mpad][slab_ld], plain stores
  int64_t slab_ld, slab_net_stride, slab_chunk_stride;
  int B, Nload;                                      // X columns < Nload are readable (the rest of the tile is zero)
  int chunk;                                         // rows of B reduced per workgroup (multiple of 64)
  int n_i_tiles;
  int reps;                                          // population: grid.z = 2 * reps, z = 2 * replica + net
  unsigned r_D, r_X, r_gather, r_slab;               // per-replica element offsets
};

// partial[chunk][net][o][i] = sum_{b in chunk} D[b][o] X[b][i].   Block tile 128(o) x 128(i), 4 waves 2x2, wave tile
// 64x64 with interleaved row/col blocks (o = base + 2*(l&31) + rb): one ds_read_b64 per operand and step feeds two MFMA
// row (column) blocks.  Both operands sit in LDS exactly as in memory (batch-row major), no transposes.  128x128 tiles
// need 32 FLOP per byte streamed from L2 (64x64 tiles: 16 FLOP/B, which demanded ~10 TB/s and stalled every stage).
// Stages are 64 batch rows (8192 MFMA cycles per wave), double buffered.  The batch axis is split over workgroups; each
// writes its partial tile with plain coalesced stores and tn_reduce_kernel sums the partials in fixed order, so weight
// gradients are bitwise reproducible (float atomics are not).
// grid: x = B chunk, y = o_tile * n_i_tiles + i_tile, z = net.
template <bool GATHER, bool POP = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) gemm_tn_kernel(const GemmTN g) {
  constexpr int TB = 64, TT = 128, LDW = TT + 4, LOADS = TB * TT / 4 / 256;  // 8 float4 per thread per operand
  extern __shared__ float lds[];
  const int z = POP ? (int)(blockIdx.z & 1u) : (int)blockIdx.z;
  const unsigned rep = POP ? blockIdx.z >> 1 : 0u;
  const int o0 = (blockIdx.y / g.n_i_tiles) * TT, i0 = (blockIdx.y % g.n_i_tiles) * TT;
  const int b_begin = blockIdx.x * g.chunk;
  const int b_end = min(b_begin + g.chunk, g.B);
  const float* __restrict__ D = g.D + (POP ? rep * g.r_D : 0u) + z * g.strideD + o0;
  const float* __restrict__ X = g.X + (POP ? rep * g.r_X : 0u) + z * g.strideX;
  const int64_t* __restrict__ gatherX = (POP && GATHER) ? g.gatherX + rep * g.r_gather : g.gatherX;   // (no arithmetic on the null pointer of GATHER = false)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int srow = tid >> 5, sc4 = tid & 31;  // staging: f = tid + 256*j -> row = srow + 8*j, c4 = sc4
  const bool x_col_ok = i0 + 4 * sc4 < g.Nload;
  const int x_col = x_col_ok ? i0 + 4 * sc4 : 0;
  const int b_last = b_end - 1;

  // Branch-free staging: out-of-range rows are clamped to the last valid row and zeroed at LDS-store time, so all 16
  // global loads of a stage are issued back to back and nothing waits on them until the stage's MFMAs are issued.
  f32x4 rd[LOADS], rx[LOADS];
#define KP1_TN_LOAD(b0)                                                                                   \
  {                                                                                                       \
    int64_t xrow[LOADS];                                                                                  \
    _Pragma("unroll") for (int j = 0; j < LOADS; ++j) {                                                   \
      const int b = min((b0) + srow + 8 * j, b_last);                                                     \
      xrow[j] = GATHER ? gatherX[b] : (int64_t)b;                                                       \
    }                                                                                                     \
    _Pragma("unroll") for (int j = 0; j < LOADS; ++j) {                                                   \
      const int b = min((b0) + srow + 8 * j, b_last);                                                     \
      rd[j] = *reinterpret_cast<const f32x4*>(D + (int64_t)b * g.ldd + 4 * sc4);                          \
      rx[j] = *reinterpret_cast<const f32x4*>(X + xrow[j] * g.ldx + x_col);                               \
    }                                                                                                     \
  }
#define KP1_TN_STORE(buf, b0)                                                                             \
  _Pragma("unroll") for (int j = 0; j < LOADS; ++j) {                                                     \
    const float keep = ((b0) + srow + 8 * j <= b_last) ? 1.f : 0.f;                                       \
    const float keepx = x_col_ok ? keep : 0.f;                                                            \
    float* base = lds + (buf) * 2 * TB * LDW + (srow + 8 * j) * LDW + 4 * sc4;                            \
    *reinterpret_cast<f32x4*>(base) = rd[j] * keep;                                                       \
    *reinterpret_cast<f32x4*>(base + TB * LDW) = rx[j] * keepx;                                           \
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[r][c][e] = 0.f;

  const int KT = (b_end - b_begin + TB - 1) / TB;
  KP1_TR(0)
  if (KT > 0) {  // uniform per workgroup
    KP1_TN_LOAD(b_begin)
    KP1_TN_STORE(0, b_begin)
    __syncthreads();
    KP1_TR(1)
    for (int kt = 0; kt < KT; ++kt) {
      const int buf = kt & 1;
      KP1_TN_LOAD(b_begin + (kt + 1) * TB)  // past the chunk end: clamped rows, zeroed at store time
      const float* ds = lds + buf * 2 * TB * LDW + (lane >> 5) * LDW + wr * 64 + 2 * (lane & 31);
      const float* xs = lds + buf * 2 * TB * LDW + TB * LDW + (lane >> 5) * LDW + wc * 64 + 2 * (lane & 31);
#pragma unroll
      for (int s0 = 0; s0 < TB / 2; s0 += 4) {
        float2 av[4], xv[4];  // LDS reads of 4 steps (16 MFMAs) in flight ahead of their use
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          av[u] = *reinterpret_cast<const float2*>(ds + 2 * (s0 + u) * LDW);
          xv[u] = *reinterpret_cast<const float2*>(xs + 2 * (s0 + u) * LDW);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].x, xv[u].x, acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].x, xv[u].y, acc[0][1], 0, 0, 0);
          acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].y, xv[u].x, acc[1][0], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].y, xv[u].y, acc[1][1], 0, 0, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);   // 8 DS reads
        __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);  // then their 16 MFMAs
      }
      KP1_TN_STORE(buf ^ 1, b_begin + (kt + 1) * TB)
      __syncthreads();
      KP1_TR(2 + (kt < 8 ? kt : 8))
    }
  }
#undef KP1_TN_LOAD
#undef KP1_TN_STORE
  // partial tile -> slab (zeros when this chunk had no rows): transposed through LDS so rows are written as float4
  constexpr int LDP = TT + 4;
  float* Ps = lds;
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int o = wr * 64 + 2 * ((e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)) + r;
        Ps[o * LDP + wc * 64 + 2 * (lane & 31) + c] = acc[r][c][e];
      }
  __syncthreads();
  KP1_TR(11)
  float* __restrict__ P = g.slab + (POP ? rep * g.r_slab : 0u) + blockIdx.x * g.slab_chunk_stride + z * g.slab_net_stride;
#pragma unroll
  for (int j = 0; j < TT * TT / 4 / 256; ++j) {
    const int f = tid + 256 * j, o = f >> 5, q = f & 31;
    const int col = i0 + 4 * q;
    if (col < g.slab_ld) *reinterpret_cast<f32x4*>(P + (int64_t)(o0 + o) * g.slab_ld + col) = *reinterpret_cast<const f32x4*>(Ps + o * LDP + 4 * q);
  }
  KP1_TR(12)
}

// ---------------------------------------------------------------------------------------------- heads
struct HeadArgs {
  const float* h2;        // [2][n][Hp]  (net 0 = policy, 1 = value)
  int64_t strideH;        // n_alloc * Hp
  int Hp, n;
  const float* w3;        // [8][Hp] rows 0..6 action_net, row 7 value_net
  const float* b3;        // [8]
  const float* log_std;   // [7]
  // inference outputs
  const float* noise; float* mean; float* value; float* action; float* clipped; float* log_prob;
  // training inputs
  const int64_t* idx; const float* actions; const float* old_logp; const float* adv; const float* ret;
  const double* adv_partials; int n_adv_partials; const float* adv_stats; float adv_mean, adv_inv_std; int adv_mode;
  float clip_range, ent_coef, vf_coef, inv_count;
  // training outputs
  float* dz2;             // [2][n][Hp]
  float* hpart;           // per-block partials [n_blocks][hpart_stride]: dW action [7][Hp], dW value [Hp], db2 pi [Hp], db2 vf [Hp],
  int hpart_stride;       //   then 8 head-bias grads, 7 log_std grads, 3 loss sums (policy, value, kl)
  int H;                  // real hidden (<= Hp)
  // population (POP kernels, grid.y = replica): activations / dz2 at + r * r_act, head partials at + r * r_hpart, advantage partials at
  // + r * r_partials, head weights at + r * 8 Hp (w3) / + r * 8 (b3, log_std), adv_stats at + 2 r; per-row inputs and outputs (idx, noise,
  // mean, value, action, clipped, log_prob) at row + r * n
  unsigned r_act, r_hpart, r_partials;
  // population with a per-replica hyper-parameter table (kp1_mlp_set_replica_hparams): [K][HP_FIELDS] floats, or NULL = the scalars above
  const float* hparams;
};

// the per-replica hyper-parameter table of a population handle: entry r = kp1_replica_hparams of replica r (include/kp1_ppo.h)
constexpr int HP_FIELDS = 6, HP_LR = 0, HP_EPS = 1, HP_MAX_NORM = 2, HP_CLIP = 3, HP_ENT = 4, HP_VF = 5;

// HeadArgs of replica `rep` of a population handle
__device__ __forceinline__ HeadArgs head_args_replica(HeadArgs a, unsigned rep) {
  const unsigned rows = rep * (unsigned)a.n, heads = rep * (unsigned)(HEADS * a.Hp);
  if (a.hparams) {   // kernarg pointer + blockIdx.y, read at kernel entry before any divergence: a uniform load once per workgroup
    const float* e = a.hparams + rep * (unsigned)HP_FIELDS;
    a.clip_range = e[HP_CLIP];
    a.vf_coef = e[HP_VF];
  }
  a.h2 += rep * a.r_act;
  a.w3 += heads; a.b3 += rep * HEADS; a.log_std += rep * HEADS;
  if (a.noise) a.noise += rows * ACT;
  if (a.mean) a.mean += rows * ACT;
  if (a.value) a.value += rows;
  if (a.action) a.action += rows * ACT;
  if (a.clipped) a.clipped += rows * ACT;
  if (a.log_prob) a.log_prob += rows;
  if (a.idx) a.idx += rows;
  if (a.adv_partials) a.adv_partials += rep * a.r_partials;
  if (a.adv_stats) a.adv_stats += 2 * rep;
  if (a.dz2) a.dz2 += rep * a.r_act;
  if (a.hpart) a.hpart += rep * a.r_hpart;
  return a;
}

constexpr int HEAD_ROWS = 32;  // rows per 256-thread block: thread = (row = t/8, out = t%8)

__device__ __forceinline__ float head_dot(const float* __restrict__ h, const float* __restrict__ w, int Hp) {
  float s = 0.f;
  for (int k = 0; k < Hp; k += 4) {
    const float4 a = *reinterpret_cast<const float4*>(h + k);
    const float4 b = *reinterpret_cast<const float4*>(w + k);
    s = fmaf(a.x, b.x, s);
    s = fmaf(a.y, b.y, s);
    s = fmaf(a.z, b.z, s);
    s = fmaf(a.w, b.w, s);
  }
  return s;
}

// policy.forward tail: heads + Gaussian sampling (SB3 DiagGaussianDistribution)
template <bool POP = false>
__global__ void __launch_bounds__(256) head_infer_kernel(const HeadArgs a_) {
  const HeadArgs a = POP ? head_args_replica(a_, blockIdx.y) : a_;
  extern __shared__ float w3s[];  // [8][Hp]
  for (int k = threadIdx.x; k < HEADS * a.Hp; k += 256) w3s[k] = a.w3[k];
  __syncthreads();
  const int row = blockIdx.x * HEAD_ROWS + (threadIdx.x >> 3), out = threadIdx.x & 7;
  const bool ok = row < a.n;
  float v = 0.f;
  if (ok) {
    const float* h = a.h2 + (out == 7 ? a.strideH : 0) + (int64_t)row * a.Hp;
    v = head_dot(h, w3s + out * a.Hp, a.Hp) + a.b3[out];
  }
  float lp = 0.f;
  if (ok && out < ACT) {
    if (a.mean) a.mean[(int64_t)row * ACT + out] = v;
    float act = v;
    if (a.noise) {
      const float ls = a.log_std[out];
      const float nz = a.noise[(int64_t)row * ACT + out];
      act = fmaf(expf(ls), nz, v);
      lp = -0.5f * nz * nz - ls - LOG_SQRT_2PI;
    }
    if (a.action) a.action[(int64_t)row * ACT + out] = act;
    if (a.clipped) a.clipped[(int64_t)row * ACT + out] = fminf(fmaxf(act, -1.f), 1.f);
  }
  if (ok && out == 7 && a.value) a.value[row] = v;
  // log_prob = sum over the 7 action lanes of the 8-lane group
  lp += __shfl_xor(lp, 1);
  lp += __shfl_xor(lp, 2);
  lp += __shfl_xor(lp, 4);
  if (ok && out == 0 && a.log_prob) a.log_prob[row] = lp;
}

// per-block partial (sum, sum of squares) of the gathered advantages, fp64, fixed order => deterministic
template <bool POP = false>
__global__ void __launch_bounds__(256) adv_partials_kernel(const float* __restrict__ adv, const int64_t* __restrict__ idx, int n, double* __restrict__ partials,
                                                           unsigned r_partials) {
  __shared__ double s1[256], s2[256];
  if constexpr (POP) {   // replica blockIdx.y: its own index row and partials
    idx += blockIdx.y * (unsigned)n;
    partials += blockIdx.y * r_partials;
  }
  double a = 0.0, b = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double v = (double)adv[idx ? idx[i] : (int64_t)i];
    a += v;
    b += v * v;
  }
  s1[threadIdx.x] = a;
  s2[threadIdx.x] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      s1[threadIdx.x] += s1[threadIdx.x + s];
      s2[threadIdx.x] += s2[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = s1[0];
    partials[2 * blockIdx.x + 1] = s2[0];
  }
}

// heads forward + PPO loss gradient + dZ2 for both nets + head weight/bias gradients
template <int HP, bool POP = false>
__global__ void __launch_bounds__(256) head_train_kernel(const HeadArgs a_) {
  const HeadArgs a = POP ? head_args_replica(a_, blockIdx.y) : a_;
  // all LDS is one dynamic array (16-B aligned base: head_dot reads float4; guide G17)
  extern __shared__ float smem[];
  const int hpitch = a.Hp + 4;             // row pitch of the staged activations: conflict-free float4 row reads
  float* w3s = smem;                       // [8][Hp]
  float* dout = smem + HEADS * a.Hp;       // [HEAD_ROWS][8] : d loss / d (mean_0..6, value)
  float* red = dout + HEAD_ROWS * 8;       // [4 waves][20] per-wave partial sums
  float* adv_ms = red + 80;                // [2] (+2 pad)
  float* h2s = adv_ms + 4;                 // [2][HEAD_ROWS][hpitch]: this block's rows of both nets, read from HBM once
  for (int k = threadIdx.x; k < HEADS * a.Hp; k += 256) w3s[k] = a.w3[k];
  {
    // all loads of this thread in flight before the first LDS store (a load->store loop serialises 16 round trips)
    constexpr int Q = HP / 4, LOADS = 2 * HEAD_ROWS * Q / 256;
    f32x4 v[LOADS];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) {
      const int f = threadIdx.x + 256 * j;
      const int net = f / (HEAD_ROWS * Q), rem = f % (HEAD_ROWS * Q), r = rem / Q, c4 = rem % Q;
      const int grow = min(blockIdx.x * HEAD_ROWS + r, a.n - 1);
      v[j] = *reinterpret_cast<const f32x4*>(a.h2 + net * a.strideH + (int64_t)grow * HP + 4 * c4);
    }
#pragma unroll
    for (int j = 0; j < LOADS; ++j) {
      const int f = threadIdx.x + 256 * j;
      const int net = f / (HEAD_ROWS * Q), rem = f % (HEAD_ROWS * Q), r = rem / Q, c4 = rem % Q;
      *reinterpret_cast<f32x4*>(h2s + (net * HEAD_ROWS + r) * hpitch + 4 * c4) = v[j];
    }
  }
#include "kp1_head_adv_body.inc"
  __syncthreads();
  const int row_l = threadIdx.x >> 3, out = threadIdx.x & 7;
  const int row = blockIdx.x * HEAD_ROWS + row_l;
  const bool ok = row < a.n;
  const int64_t src = ok ? (a.idx ? a.idx[row] : (int64_t)row) : 0;
  float v = 0.f;
  if (ok) v = head_dot(h2s + ((out == 7 ? HEAD_ROWS : 0) + row_l) * hpitch, w3s + out * a.Hp, a.Hp) + a.b3[out];
#include "kp1_head_loss_body.inc"
  __syncthreads();
  float* part = a.hpart + (int64_t)blockIdx.x * a.hpart_stride;
  if (threadIdx.x < 18) {
    const int k = threadIdx.x;  // 0..7 bias grads, 8..14 log_std grads, 15..17 loss sums
    const int slot = k < 8 ? 4 + k : (k < 15 ? 12 + (k - 8) : k - 15);
    part[10 * a.Hp + k] = ((red[slot] + red[20 + slot]) + red[40 + slot]) + red[60 + slot];
  }
  // phase 2: one thread per hidden column; dZ2 = (dOut W3) * (1 - h2^2), head weight grads, layer-2 bias grads
  const int rows_here = min(HEAD_ROWS, a.n - blockIdx.x * HEAD_ROWS);
  for (int h = threadIdx.x; h < a.Hp; h += 256) {
    float wcol[HEADS];
#pragma unroll
    for (int o = 0; o < HEADS; ++o) wcol[o] = w3s[o * a.Hp + h];
    float gw[HEADS];
#pragma unroll
    for (int o = 0; o < HEADS; ++o) gw[o] = 0.f;
    float gb2p = 0.f, gb2v = 0.f;
    for (int r = 0; r < rows_here; ++r) {
      const int64_t rr = (int64_t)(blockIdx.x * HEAD_ROWS + r) * a.Hp + h;
      const float hp = h2s[r * hpitch + h], hv = h2s[(HEAD_ROWS + r) * hpitch + h];
      float dp = 0.f;
#pragma unroll
      for (int o = 0; o < ACT; ++o) {
        const float dd = dout[r * 8 + o];
        dp = fmaf(dd, wcol[o], dp);
        gw[o] = fmaf(dd, hp, gw[o]);
      }
      const float dv = dout[r * 8 + 7];
      gw[7] = fmaf(dv, hv, gw[7]);
      const float dzp = dp * (1.f - hp * hp);
      const float dzv = dv * wcol[7] * (1.f - hv * hv);
      a.dz2[rr] = dzp;
      a.dz2[a.strideH + rr] = dzv;
      gb2p += dzp;
      gb2v += dzv;
    }
#pragma unroll
    for (int o = 0; o < HEADS; ++o) part[o * a.Hp + h] = gw[o];
    part[8 * a.Hp + h] = gb2p;
    part[9 * a.Hp + h] = gb2v;
  }
}

// ---------------------------------------------------------------------------------------------- optimiser
struct ParamLayout {  // offsets into the flat SB3-order vector
  int H, Hp, IN, INP;  // INP: IN rounded up to the k depth the GEMMs are instantiated for (64 or 128)
  int64_t log_std, p_w1, p_b1, p_w2, p_b2, v_w1, v_b1, v_w2, v_b2, a_w, a_b, c_w, c_b, total;
};

__host__ __device__ inline ParamLayout make_layout(int H, int IN = KP1_MLP_IN) {
  ParamLayout L;
  L.H = H;
  L.IN = IN;
  L.INP = IN <= 64 ? 64 : 128;
  L.Hp = (H + 127) / 128 * 128;
  int64_t o = 0;
  L.log_std = o; o += ACT;
  L.p_w1 = o; o += (int64_t)H * IN;
  L.p_b1 = o; o += H;
  L.p_w2 = o; o += (int64_t)H * H;
  L.p_b2 = o; o += H;
  L.v_w1 = o; o += (int64_t)H * IN;
  L.v_b1 = o; o += H;
  L.v_w2 = o; o += (int64_t)H * H;
  L.v_b2 = o; o += H;
  L.a_w = o; o += (int64_t)ACT * H;
  L.a_b = o; o += ACT;
  L.c_w = o; o += H;
  L.c_b = o; o += 1;
  L.total = o;
  return L;
}

// Kernel-format GEMM weights are "k-slab major": W[net][K/32][N][32], i.e. element (out row n, in column k) of a net sits
// at (k/32)*N*32 + n*32 + k%32.  One 32-deep W stage of a GEMM is then ONE contiguous N*128-byte run.  With the natural
// row-major [N][K] layout a stage is N separate 128-byte pieces at a 1 KB pitch, which (256-byte channel interleave) land
// on 4 of the 16 L2 channels of an XCD -- every CU streams the same stage at the same time, and the MFMA loops of all
// three GEMM kinds sat at ~50 % waiting on those four channels.
// The fused tile kernel reads a second copy, "fragment major": inside each 32-deep k stage the order is [MFMA column block
// n/32][k group (k%32)/8][lane = n%32 + 32*((k%8)/4)][k%4] -- exactly the float4 every lane feeds to four consecutive
// v_mfma_f32_32x32x2_f32 as B operand, so the weights go global -> VGPR in coalesced 1 KB wave loads, never through LDS.
struct Packed {
  float *w1p, *b1, *w2, *w2t, *b2, *w3, *b3, *log_std;  // [2][2][Hp][32], [2][Hp], [2][Hp/32][Hp][32] x2, [2][Hp], [8][Hp], [8], [8]
  float *w1f, *w2f, *w2tf;                               // fragment-major copies of w1p, w2, w2t
  int formats;                                           // which GEMM-weight copies pack_one writes: bit 0 k-slab major, bit 1 fragment major
};
constexpr int PACK_SLAB = 1, PACK_FRAG = 2;
__host__ __device__ inline int64_t slab_at(int64_t n, int64_t k, int64_t N) { return (k >> 5) * N * 32 + n * 32 + (k & 31); }
__host__ __device__ inline int64_t frag_at(int64_t n, int64_t k, int64_t N) {
  return (k >> 5) * N * 32 + (n >> 5) * 1024 + ((k & 31) >> 3) * 256 + ((n & 31) + 32 * ((k & 7) >> 2)) * 4 + (k & 3);
}

// flat SB3 vector element i -> its place(s) in the kernel-format weights (zero padding pre-set once at creation)
__device__ __forceinline__ void pack_one(int64_t i, float v, const ParamLayout& L, const Packed& k) {
  // 32-bit element offsets and unsigned divisions: a 64-bit signed division is a ~100-instruction software routine on this ISA and sat on the
  // per-thread critical path of adam_kernel (the vector has < 2^31 elements)
  const int H = L.H, Hp = L.Hp, IN = L.IN, INP = L.INP;
  const unsigned uH = (unsigned)H, uIN = (unsigned)IN;
  if (i < L.p_w1) {
    k.log_std[i] = v;
  } else if (i < L.p_b1) {
    const unsigned e = (unsigned)(i - L.p_w1), r = e / uIN, c = e - r * uIN;
    if (k.formats & PACK_SLAB) k.w1p[slab_at(r, c, Hp)] = v;
    if (k.formats & PACK_FRAG) k.w1f[frag_at(r, c, Hp)] = v;
  } else if (i < L.p_w2) {
    k.b1[i - L.p_b1] = v;
  } else if (i < L.p_b2) {
    const unsigned e = (unsigned)(i - L.p_w2), r = e / uH, c = e - r * uH;
    if (k.formats & PACK_SLAB) {
      k.w2[slab_at(r, c, Hp)] = v;
      k.w2t[slab_at(c, r, Hp)] = v;
    }
    if (k.formats & PACK_FRAG) {
      k.w2f[frag_at(r, c, Hp)] = v;
      k.w2tf[frag_at(c, r, Hp)] = v;
    }
  } else if (i < L.v_w1) {
    k.b2[i - L.p_b2] = v;
  } else if (i < L.v_b1) {
    const unsigned e = (unsigned)(i - L.v_w1), r = e / uIN, c = e - r * uIN;
    if (k.formats & PACK_SLAB) k.w1p[(int64_t)Hp * INP + slab_at(r, c, Hp)] = v;
    if (k.formats & PACK_FRAG) k.w1f[(int64_t)Hp * INP + frag_at(r, c, Hp)] = v;
  } else if (i < L.v_w2) {
    k.b1[Hp + i - L.v_b1] = v;
  } else if (i < L.v_b2) {
    const unsigned e = (unsigned)(i - L.v_w2), r = e / uH, c = e - r * uH;
    if (k.formats & PACK_SLAB) {
      k.w2[(int64_t)Hp * Hp + slab_at(r, c, Hp)] = v;
      k.w2t[(int64_t)Hp * Hp + slab_at(c, r, Hp)] = v;
    }
    if (k.formats & PACK_FRAG) {
      k.w2f[(int64_t)Hp * Hp + frag_at(r, c, Hp)] = v;
      k.w2tf[(int64_t)Hp * Hp + frag_at(c, r, Hp)] = v;
    }
  } else if (i < L.a_w) {
    k.b2[Hp + i - L.v_b2] = v;
  } else if (i < L.a_b) {
    const unsigned e = (unsigned)(i - L.a_w), r = e / uH;
    k.w3[(int64_t)r * Hp + (e - r * uH)] = v;
  } else if (i < L.c_w) {
    k.b3[i - L.a_b] = v;
  } else if (i < L.c_b) {
    k.w3[(int64_t)7 * Hp + (i - L.c_w)] = v;
  } else {
    k.b3[7] = v;
  }
}

// the kernel-format weights of replica `rep` of a population handle: every array holds one copy per replica back to back
__device__ __forceinline__ Packed packed_replica(Packed k, const ParamLayout& L, unsigned rep) {
  const unsigned hp = (unsigned)L.Hp, w1 = rep * 2u * hp * (unsigned)L.INP, w2 = rep * 2u * hp * hp, b = rep * 2u * hp;
  k.w1p += w1; k.w1f += w1;
  k.w2 += w2; k.w2t += w2; k.w2f += w2; k.w2tf += w2;
  k.b1 += b; k.b2 += b;
  k.w3 += rep * (unsigned)HEADS * hp;
  k.b3 += rep * (unsigned)HEADS; k.log_std += rep * (unsigned)HEADS;
  return k;
}

// POP: grid.y = replica, params [K][total]
template <bool POP = false>
__global__ void __launch_bounds__(256) pack_kernel(const float* __restrict__ p, const ParamLayout L, const Packed k) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if constexpr (POP) {
    if (i < L.total) pack_one(i, p[blockIdx.y * (unsigned)L.total + i], L, packed_replica(k, L, blockIdx.y));
  } else {
    if (i < L.total) pack_one(i, p[i], L, k);
  }
}

// Gradient finalisation: every producer kernel (TN GEMMs, backward-GEMM epilogue, head kernel) wrote per-workgroup
// partials with plain stores; this kernel sums them in a fixed order into the flat SB3-order gradient, adds the entropy
// term, accumulates the loss statistics and (fused) the per-block sum of squares for clip_grad_norm_.  No float atomics
// touch a gradient anywhere, so results are bitwise reproducible run to run.
struct FinalizeArgs {
  ParamLayout L;
  const float* slab2; int64_t s2_ld, s2_net, s2_chunk; int s2_n;   // dW2 partials [chunk][net][Hp][Hp]
  const float* slab1; int64_t s1_ld, s1_net, s1_chunk; int s1_n;   // dW1 partials [chunk][net][Hp][64]
  const float* bslab; int64_t b_net, b_tile; int b_n;              // db1 partials [row tile][net][Hp]
  const float* hpart; int64_t h_stride; int h_n;                   // head partials [block][10 Hp + 18]
  float ent_coef, inv_count;
  const float* log_std;
  float* grad; float* stats; double* sumsq;
  int* step_counter;  // Adam step counts kept on the device, kp1_mlp::step_dev (hipGraph replays cannot change a scalar kernel argument)
  // population (POP kernel, grid.y = replica): partials at + r * r_*, grad at + r * total, stats at + 4 r, log_std at + 8 r; the shared
  // step counter is advanced by replica 0 only
  unsigned r_slab2, r_slab1, r_bslab, r_hpart, r_sumsq;
  const float* hparams;   // per-replica hyper-parameter table [K][HP_FIELDS] or NULL (ent_coef above); POP kernel only
};

__device__ __forceinline__ FinalizeArgs finalize_args_replica(FinalizeArgs a, unsigned rep) {
  if (a.hparams) a.ent_coef = a.hparams[rep * (unsigned)HP_FIELDS + HP_ENT];   // uniform load at kernel entry
  a.slab2 += rep * a.r_slab2; a.slab1 += rep * a.r_slab1; a.bslab += rep * a.r_bslab; a.hpart += rep * a.r_hpart;
  a.log_std += rep * (unsigned)HEADS;
  a.grad += rep * (unsigned)a.L.total;
  if (a.stats) a.stats += 4u * rep;
  a.sumsq += rep * a.r_sumsq;
  if (rep != 0) a.step_counter = nullptr;
  return a;
}

// kp1_mlp::step_dev (STEP_DEV_INTS ints, one 64-byte line).  [CNT_STEP] is the common Adam step count and [CNT_EXTRA] the steps the actor
// tensors have taken beyond it.  Behind them sits the Adam record: the bias corrections of exactly the counts named in its tags, written once
// per optimiser step by the one thread that advances a count (grad_finalize_kernel, anchor_count_kernel) or that knows the count the next
// Adam launch will use (anchor_finalize_kernel), so that no thread of an Adam launch evaluates a powf.  An Adam launch whose counts differ
// from the tags (the host set a count in between, a step count given by the caller) evaluates the same expressions itself.
constexpr int CNT_STEP = 0, CNT_EXTRA = 1;
constexpr int REC_STEP = 4, REC_EXTRA = 5, REC_BC = 6;      // tags, then bc1, bc2_sqrt, bc1 (actor), bc2_sqrt (actor) as floats
constexpr int AREC_ST = 10, AREC_BC2 = 11, AREC_BC1 = 12;   // anchor_adam_kernel: its step tag, sqrt(1 - 0.999^st) (float), 1 - 0.9^st (double)
constexpr int STEP_DEV_INTS = 16;
static_assert(REC_BC + 4 == AREC_ST && AREC_BC1 % 2 == 0 && AREC_BC1 + 2 <= STEP_DEV_INTS, "the record's fields");

// the bias corrections of torch.optim.Adam at an fp32 step count: the one text of these expressions, for the record and for the launches
// that evaluate them in place
__device__ __forceinline__ void adam_bias(float step, float& bc1, float& bc2_sqrt) {
  bc1 = 1.f - powf(0.9f, step);
  bc2_sqrt = sqrtf(1.f - powf(0.999f, step));
}
// the actor tensors' pair: the common one unless they have taken `extra` more steps (torch keeps one count per tensor)
__device__ __forceinline__ void adam_bias_actor(float step, int extra, float bc1, float bc2_sqrt, float& bc1_a, float& bc2_sqrt_a) {
  bc1_a = bc1; bc2_sqrt_a = bc2_sqrt;
  if (extra != 0) adam_bias(step + (float)extra, bc1_a, bc2_sqrt_a);
}
__device__ __forceinline__ void adam_record_write(int* cnt, int step, int extra) {
  float bc[4];
  adam_bias((float)step, bc[0], bc[1]);
  adam_bias_actor((float)step, extra, bc[0], bc[1], bc[2], bc[3]);
#pragma unroll
  for (int q = 0; q < 4; ++q) cnt[REC_BC + q] = __float_as_int(bc[q]);
  cnt[REC_STEP] = step; cnt[REC_EXTRA] = extra;
}
// anchor_adam_kernel forms its corrections in f64 at st = common + actor extra + 1 (see there)
__device__ __forceinline__ double anchor_bias1(int st) { return 1.0 - pow(0.9, (double)st); }
__device__ __forceinline__ float anchor_bias2_sqrt(int st) { return (float)sqrt(1.0 - pow(0.999, (double)st)); }

template <int UNROLL>
__device__ __forceinline__ float sum_strided(const float* __restrict__ p, int64_t stride, int n) {
  float s = 0.f;
  int c = 0;
  for (; c + UNROLL <= n; c += UNROLL) {
    float v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) v[u] = p[(int64_t)(c + u) * stride];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) s += v[u];
  }
  for (; c < n; ++c) s += p[(int64_t)c * stride];
  return s;
}

// where the partials of flat gradient element i live: n values at p[c * stride], plus a constant
struct PartialSrc {
  const float* p; int64_t stride; int n; float add;
  bool wide;  // few elements with one partial per 32-row tile (biases, heads, log_std): summed cooperatively
};

__device__ __forceinline__ PartialSrc finalize_source(const FinalizeArgs& a, int64_t i) {
  const ParamLayout& L = a.L;
  const int H = L.H, Hp = L.Hp, IN = L.IN;
  PartialSrc r;
  r.add = 0.f;
  r.wide = true;
  r.stride = a.h_stride;
  r.n = a.h_n;
  if (i < L.p_w1) {
    r.p = a.hpart + 10 * Hp + 8 + i;
    r.add = -a.ent_coef;  // d(-ent_coef * sum log_std)
  } else if (i < L.p_b1 || (i >= L.v_w1 && i < L.v_b1)) {
    const int net = i >= L.v_w1;
    const int64_t e = i - (net ? L.v_w1 : L.p_w1);
    r.p = a.slab1 + net * a.s1_net + (e / IN) * a.s1_ld + e % IN;
    r.stride = a.s1_chunk; r.n = a.s1_n; r.wide = false;
  } else if (i < L.p_w2 || (i >= L.v_b1 && i < L.v_w2)) {
    const int net = i >= L.v_b1;
    r.p = a.bslab + net * a.b_net + (i - (net ? L.v_b1 : L.p_b1));
    r.stride = a.b_tile; r.n = a.b_n;
  } else if (i < L.p_b2 || (i >= L.v_w2 && i < L.v_b2)) {
    const int net = i >= L.v_w2;
    const int64_t e = i - (net ? L.v_w2 : L.p_w2);
    r.p = a.slab2 + net * a.s2_net + (e / H) * a.s2_ld + e % H;
    r.stride = a.s2_chunk; r.n = a.s2_n; r.wide = false;
  } else if (i < L.v_w1) {
    r.p = a.hpart + 8 * Hp + (i - L.p_b2);
  } else if (i < L.a_w) {
    r.p = a.hpart + 9 * Hp + (i - L.v_b2);
  } else if (i < L.a_b) {
    const int64_t e = i - L.a_w;
    r.p = a.hpart + (e / H) * Hp + e % H;
  } else if (i < L.c_w) {
    r.p = a.hpart + 10 * Hp + (i - L.a_b);
  } else if (i < L.c_b) {
    r.p = a.hpart + 7 * Hp + (i - L.c_w);
  } else {
    r.p = a.hpart + 10 * Hp + 7;
  }
  return r;
}

// the "wide" elements in enumeration order: log_std, pi b1, pi b2, vf b1, vf b2, then everything from action_net on
__host__ __device__ inline int64_t finalize_wide_count(const ParamLayout& L) { return ACT + 4 * (int64_t)L.H + (L.total - L.a_w); }
__device__ __forceinline__ int64_t finalize_wide_index(const ParamLayout& L, int64_t e) {
  const int H = L.H;
  if (e < ACT) return L.log_std + e;
  e -= ACT;
  if (e < H) return L.p_b1 + e;
  e -= H;
  if (e < H) return L.p_b2 + e;
  e -= H;
  if (e < H) return L.v_b1 + e;
  e -= H;
  if (e < H) return L.v_b2 + e;
  e -= H;
  return L.a_w + e;
}

// Blocks [0, n_main): the four weight matrices (dW2, dW1 of both nets; few partials per element: one per batch chunk of the TN GEMMs).
// One thread owns FOUR consecutive columns of one weight row and sums its float4 partials over the chunks with all loads in flight: a
// quarter of the load instructions of a thread-per-element walk over the same 25 MB (the kernel is bound by load issue + latency, not
// bandwidth), same summation order per element (chunk 0, 1, 2, ...).  Blocks [n_main, ...): 32 "wide" elements each (biases, heads,
// log_std: one partial per 32-row tile), 8 threads per element walk the per-tile partials with a stride of 8 (32 loads in flight each) and
// LDS combines the 8 strands in a fixed order -- a single thread summing 256 tiles was the tail of this kernel (8 dependent load rounds).
// Every block leaves the sum of squares of what it wrote in sumsq[blockIdx.x] for clip_grad_norm_.
__host__ __device__ inline int64_t finalize_vec_items(const ParamLayout& L) { return 2 * ((int64_t)L.H * L.H / 4 + (int64_t)L.H * L.IN / 4); }
// (a form with 2 or 4 lanes splitting the chunks of one item was measured and removed: DESIGN.md 4.3)

//
// GATE (grad_finalize_gated_kernel): the KL early stop of SB3's PPO.train() as a device decision.  `gate` holds one
// kp1_kl_gate per replica and a_.step_counter one STEP_DEV_INTS line per replica.  All four statistics of a minibatch are owned by lanes of
// wave 0 of ONE wide block (the three loss sums and, in this form, the entropy term: finalize_gate_layout_ok), and the lane of the KL sum
// decides there: nothing else in the launch that takes the decision reads it, every later launch does.  The gradient and the norm partials
// are written whatever the gate says.
__host__ __device__ inline bool finalize_gate_layout_ok(const ParamLayout& L) { return finalize_wide_count(L) % 32 + 3 < 32; }

template <bool POP = false>
__global__ void __launch_bounds__(256) grad_finalize_kernel(const FinalizeArgs a_, int n_main) {
  constexpr bool GATE = false;
  constexpr kp1_kl_gate* gate = nullptr;
#include "kp1_grad_finalize_body.inc"
}
template <bool POP = false>
__global__ void __launch_bounds__(256) grad_finalize_gated_kernel(const FinalizeArgs a_, int n_main, kp1_kl_gate* gate) {
  constexpr bool GATE = true;
#include "kp1_grad_finalize_body.inc"
}

#ifndef KP1_MLP_LINE_TU   // a kernel that is no template is emitted wherever it is read: not into kp1_mlp_line.hip's code object
// kp1_mlp_kl_gate_arm: a new train() call begins; the thresholds stay
__global__ void kl_gate_arm_kernel(kp1_kl_gate* __restrict__ gate, int n) {
  const int r = (int)threadIdx.x;
  if (r < n) {
    gate[r].stopped = 0; gate[r].n_counted = 0; gate[r].n_seen = 0; gate[r].stop_index = 0; gate[r].stop_kl = 0.f;
  }
}
#endif

template <bool POP = false>
__global__ void __launch_bounds__(256) sumsq_partials_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partials, unsigned r_partials) {
  __shared__ double s[256];
  if constexpr (POP) {   // replica blockIdx.y: grad [K][n]
    g += blockIdx.y * (unsigned)n;
    partials += blockIdx.y * r_partials;
  }
  double a = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) a += (double)g[i] * (double)g[i];
  s[threadIdx.x] = a;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) s[threadIdx.x] += s[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = s[0];
}

// torch.nn.utils.clip_grad_norm_ (coef = max_norm / (norm + 1e-6), clamped to 1) + torch.optim.Adam
// The same pass repacks the updated element into the kernel-format weights and (zero_grad) clears the gradient, so the
// next minibatch's atomic accumulation starts from zero without a memset launch.
// One thread per element: a float4-per-thread form measured SLOWER (8.1 -> 12.9 us in situ, profiles/r02_ab_adam_vec4.log): the kernel is a
// latency chain per thread (scattered repack stores behind div / sqrt), so it wants more threads, not fatter ones.
// (The loops over VEC = 1 are one trip.  Written without them -- one `i`, its `i < n` shared by the load clamp and the store guard -- the kernel
// compiles to a different register assignment and load order than the measured one, so this form is kept.)
// POP: grid.y = replica; p, g, m, v are [K][n], the norm partials of replica r sit at + r * r_partials, one clip norm per replica, one
// shared step count
constexpr int ADAM_BLOCK = 256, VEC = 1, NORM_BATCH = 4;
// The sum of the norm partials, by one whole wave: lane l owns q = l, l + 64, ... and adds them in that order, NORM_BATCH of them in flight
// before the first add, then the xor tree.  A load past the end reads the last partial and adds +0.0, which leaves a non-negative sum as it
// is.  (A plain `q += 64` loop compiles to load, wait, add, branch: one exposed memory round trip per 64 partials, in front of the barrier every
// thread of the workgroup waits at.)
__device__ __forceinline__ double norm_partials_sum(const double* __restrict__ partials, int n_partials) {
  double s = 0.0;
  for (int q0 = threadIdx.x; q0 < n_partials; q0 += 64 * NORM_BATCH) {
    double t[NORM_BATCH];
#pragma unroll
    for (int u = 0; u < NORM_BATCH; ++u) t[u] = partials[min(q0 + 64 * u, n_partials - 1)];
#pragma unroll
    for (int u = 0; u < NORM_BATCH; ++u) s += q0 + 64 * u < n_partials ? t[u] : 0.0;
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}
// GATE (adam_gated_kernel): `cnt` holds one line per replica, and a replica whose gate has stopped leaves before any store -- parameters,
// moments and packed weights stay as the last step taken left them.
template <bool POP = false>
__global__ void __launch_bounds__(ADAM_BLOCK) adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   int64_t n, const double* __restrict__ partials, int n_partials, int host_step,
                                                   const int* __restrict__ cnt, float lr, float eps, float max_norm, float bc1, float bc2_sqrt,
                                                   int zero_grad, unsigned r_partials, const float* __restrict__ hparams, const ParamLayout L,
                                                   const Packed k_) {
  constexpr bool GATE = false;
  constexpr const kp1_kl_gate* gate = nullptr;
#include "kp1_adam_body.inc"
}
template <bool POP = false>
__global__ void __launch_bounds__(ADAM_BLOCK) adam_gated_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   int64_t n, const double* __restrict__ partials, int n_partials, int host_step,
                                                   const int* __restrict__ cnt, float lr, float eps, float max_norm, float bc1, float bc2_sqrt,
                                                   int zero_grad, unsigned r_partials, const float* __restrict__ hparams, const ParamLayout L,
                                                   const Packed k_, const kp1_kl_gate* __restrict__ gate) {
  constexpr bool GATE = true;
#include "kp1_adam_body.inc"
}

// ---------------------------------------------------------------------------------------------- teacher-anchor side loss
// loss = loss_weight * mean_{i < n, d < 7} (mean(obs[idx[i]])_d - teacher[idx[i]][d])^2 on the unclipped policy mean (the route trainer's
// RouteTeacherAnchorCallback).  Only the policy net and action_net get a gradient; the forward layers, dZ1 and the weight-gradient GEMMs are
// the layer-wise launches of kp1_mlp_loss_grad, the head, the finalize and the Adam step are the kernels below.
struct AnchorHeadArgs {
  const float* h2;        // [2][n][HP]
  int64_t strideH;
  int n;
  const float* w3;        // [8][HP]
  const float* b3;        // [8]
  const int64_t* idx;     // rows of the teacher dataset (NULL: rows 0..n)
  const float* teacher;   // [M][7]
  float dcoef, lcoef;     // loss_weight * 2 / (7 n), loss_weight / (7 n)
  float* dz2;             // [2][n][HP]
  float* hpart;           // head_train_kernel's layout: dW action at [o][HP], db2 pi at 8 HP, head-bias grads at 10 HP, the loss sum at 10 HP + 15
  int hpart_stride;
  unsigned r_act, r_hpart;   // POP: grid.y = replica
};

// head_train_kernel's shape for the anchor loss: 32 rows per 256-thread block, w3 and the block's policy-net h2 rows staged in LDS once (all
// loads in flight before the first LDS store), thread = (row, out) for d loss / d mean, then one thread per hidden column for the policy
// net's dZ2 tile and the action_net partials; the value net's dZ2 tile is written as zeros (its gradient GEMMs then produce zeros).
template <int HP, bool POP = false>
__global__ void __launch_bounds__(256) head_anchor_kernel(const AnchorHeadArgs a_) {
  AnchorHeadArgs a = a_;
  if constexpr (POP) {
    const unsigned rep = blockIdx.y;
    a.h2 += rep * a.r_act; a.dz2 += rep * a.r_act; a.hpart += rep * a.r_hpart;
    a.w3 += rep * (unsigned)(HEADS * HP); a.b3 += rep * (unsigned)HEADS;
    if (a.idx) a.idx += rep * (unsigned)a.n;
  }
  // all LDS is one dynamic array (16-B aligned base; every carve below is a multiple of 4 floats: head_dot reads float4)
  extern __shared__ float smem[];
  constexpr int hpitch = HP + 4, Q = HP / 4, LOADS = HEAD_ROWS * Q / 256, WLOADS = HEADS * Q / 256;
  static_assert(HEAD_ROWS * Q % 256 == 0 && HEADS * Q % 256 == 0 && 2 * HP % 256 == 0, "head_anchor_kernel staging");
  float* w3s = smem;                        // [8][HP]
  float* dout = smem + HEADS * HP;          // [HEAD_ROWS][8]: d loss / d mean_0..6 (slot 7 = 0)
  float* red = dout + HEAD_ROWS * 8;        // [4 waves][12]: 7 bias grads, pad, the loss sum at +8
  float* h2s = red + 48;                    // [HEAD_ROWS][hpitch]
  {
    f32x4 wv[WLOADS], hv[LOADS];
#pragma unroll
    for (int j = 0; j < WLOADS; ++j) wv[j] = *reinterpret_cast<const f32x4*>(a.w3 + 4 * (threadIdx.x + 256 * j));
#pragma unroll
    for (int j = 0; j < LOADS; ++j) {
      const int f = threadIdx.x + 256 * j, r = f / Q, c4 = f % Q;
      const int grow = min(blockIdx.x * HEAD_ROWS + r, a.n - 1);
      hv[j] = *reinterpret_cast<const f32x4*>(a.h2 + (int64_t)grow * HP + 4 * c4);
    }
#pragma unroll
    for (int j = 0; j < WLOADS; ++j) *reinterpret_cast<f32x4*>(w3s + 4 * (threadIdx.x + 256 * j)) = wv[j];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) {
      const int f = threadIdx.x + 256 * j, r = f / Q, c4 = f % Q;
      *reinterpret_cast<f32x4*>(h2s + r * hpitch + 4 * c4) = hv[j];
    }
  }
  __syncthreads();
  const int row_l = threadIdx.x >> 3, out = threadIdx.x & 7;
  const int row = blockIdx.x * HEAD_ROWS + row_l;
  const bool ok = row < a.n && out < ACT;     // tail rows and the eighth lane of a row contribute 0
  float d = 0.f, l = 0.f;
  if (ok) {
    const int64_t src = a.idx ? a.idx[row] : (int64_t)row;
    const float mean = head_dot(h2s + row_l * hpitch, w3s + out * HP, HP) + a.b3[out];
    const float diff = mean - a.teacher[src * ACT + out];
    d = a.dcoef * diff;
    l = a.lcoef * diff * diff;
  }
  dout[row_l * 8 + out] = d;
  // per-wave sums (lanes with equal t & 7 hold the same `out`; the loss over the whole wave), combined across the 4 waves in a fixed order
  float dsum = d;
  dsum += __shfl_xor(dsum, 8);
  dsum += __shfl_xor(dsum, 16);
  dsum += __shfl_xor(dsum, 32);
  float lsum = l;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) lsum += __shfl_xor(lsum, off);
  const int wave_ = threadIdx.x >> 6;
  if ((threadIdx.x & 63) < 8) red[wave_ * 12 + out] = dsum;
  if ((threadIdx.x & 63) == 0) red[wave_ * 12 + 8] = lsum;
  __syncthreads();
  float* part = a.hpart + (int64_t)blockIdx.x * a.hpart_stride;
  if (threadIdx.x < 8) {   // 0..6 action_net bias grads, 7 the loss
    const int slot = threadIdx.x < ACT ? threadIdx.x : 8;
    part[10 * HP + (threadIdx.x < ACT ? threadIdx.x : 15)] = ((red[slot] + red[12 + slot]) + red[24 + slot]) + red[36 + slot];
  }
  // phase 2: threads [0, HP) own one hidden column of the policy net, threads [HP, 2 HP) zero the same column of the value net's dZ2
  const int rows_here = min(HEAD_ROWS, a.n - blockIdx.x * HEAD_ROWS);
  for (int hh = threadIdx.x; hh < 2 * HP; hh += 256) {
    const int h = hh % HP;
    if (hh >= HP) {
      for (int r = 0; r < rows_here; ++r) a.dz2[a.strideH + (int64_t)(blockIdx.x * HEAD_ROWS + r) * HP + h] = 0.f;
      continue;
    }
    float wcol[ACT], gw[ACT];
#pragma unroll
    for (int o = 0; o < ACT; ++o) {
      wcol[o] = w3s[o * HP + h];
      gw[o] = 0.f;
    }
    float gb2 = 0.f;
    for (int r = 0; r < rows_here; ++r) {
      const float hp = h2s[r * hpitch + h];
      float dp = 0.f;
#pragma unroll
      for (int o = 0; o < ACT; ++o) {
        const float dd = dout[r * 8 + o];
        dp = fmaf(dd, wcol[o], dp);
        gw[o] = fmaf(dd, hp, gw[o]);
      }
      const float dz = dp * (1.f - hp * hp);
      a.dz2[(int64_t)(blockIdx.x * HEAD_ROWS + r) * HP + h] = dz;
      gb2 += dz;
    }
#pragma unroll
    for (int o = 0; o < ACT; ++o) part[o * HP + h] = gw[o];
    part[8 * HP + h] = gb2;
  }
}

__device__ __forceinline__ bool is_actor_element(const ParamLayout& L, int64_t i) {
  return (i >= L.p_w1 && i < L.v_w1) || (i >= L.a_w && i < L.c_w);   // policy_net.{0,2}.{weight,bias}, action_net.{weight,bias}
}

// The anchor gradient in SB3 order: an actor element is the fixed-order sum of its producers' partials (finalize_source: the same places
// grad_finalize_kernel reads), every other element is written as 0.  Block b leaves the f64 sum of squares of what it wrote in sumsq[b]
// (the norm of the six actor tensors: the rest is zero), thread 0 of block 0 sums the loss partials.  Does not touch the step count: it
// reads the counts and leaves the bias corrections of the Adam launch that follows in the record behind them.
struct AnchorFinalizeArgs {
  FinalizeArgs f;      // stats, hparams unused (NULL); step_counter = the handle's counts, read only; sumsq = the handle's anchor partials
  float* loss_out;     // [K]
};

template <bool POP = false>
__global__ void __launch_bounds__(256) anchor_finalize_kernel(const AnchorFinalizeArgs a_) {
  const FinalizeArgs a = POP ? finalize_args_replica(a_.f, blockIdx.y) : a_.f;
  const ParamLayout& L = a.L;
  __shared__ double sq[4];
  const int64_t i = (int64_t)(blockIdx.x * 256u + threadIdx.x);
  float gval = 0.f;
  if (i < L.total) {
    if (is_actor_element(L, i)) {
      const PartialSrc s = finalize_source(a, i);
      for (int c = 0; c < s.n; ++c) gval += s.p[(int64_t)c * s.stride];
    }
    a.grad[i] = gval;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // element 0 is log_std: this thread has no gradient to sum
    float t = 0.f;
    for (int c = 0; c < a.h_n; ++c) t += a.hpart[(int64_t)c * a.h_stride + 10 * L.Hp + 15];
    a_.loss_out[POP ? blockIdx.y : 0u] = t;
  }
  // the bias corrections of the anchor_adam_kernel launch that follows, on the device's counts (replica 0, in another wave than the loss sum)
  if (a.step_counter && blockIdx.x == 0 && threadIdx.x == 64) {
    int* cnt = a.step_counter;
    const int st = cnt[CNT_STEP] + cnt[CNT_EXTRA] + 1;
    *reinterpret_cast<double*>(cnt + AREC_BC1) = anchor_bias1(st);
    cnt[AREC_BC2] = __float_as_int(anchor_bias2_sqrt(st));
    cnt[AREC_ST] = st;
  }
  double w = (double)gval * (double)gval;
  for (int off = 32; off > 0; off >>= 1) w += __shfl_xor(w, off);
  if ((threadIdx.x & 63) == 0) sq[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) a.sumsq[blockIdx.x] = ((sq[0] + sq[1]) + sq[2]) + sq[3];
}

// clip_grad_norm_(max_norm) over the actor tensors + torch.optim.Adam on the actor ranges only, with the per-tensor step count
// common + actor_extra + 1 (common = host_step, or the device counter when host_step <= 0); the changed elements are repacked in the same
// pass.  Nothing outside the actor ranges is written.  The bias corrections are formed once per block in f64, as the host-side torch step
// forms them (step size lr / (1 - 0.9^t) and sqrt(1 - 0.999^t) rounded to fp32).  POP: grid.y = replica; lr / eps from the table when set.
template <bool POP = false>
__global__ void __launch_bounds__(ADAM_BLOCK) anchor_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                          const double* __restrict__ partials, int n_partials, float lr, float eps, float max_norm,
                                                          const ParamLayout L, const Packed k_, const int* __restrict__ step_dev, int host_step,
                                                          unsigned r_partials, const float* __restrict__ hparams) {
  __shared__ float sh[3];   // clip scale, lr / bc1, sqrt(bc2)
  const Packed k = POP ? packed_replica(k_, L, blockIdx.y) : k_;
  if constexpr (POP) {
    const unsigned o = blockIdx.y * (unsigned)L.total;
    p += o; g += o; m += o; v += o;
    partials += blockIdx.y * r_partials;
    if (hparams) {
      const float* e = hparams + blockIdx.y * (unsigned)HP_FIELDS;
      lr = e[HP_LR];
      eps = e[HP_EPS];
    }
  }
  const int64_t i = (int64_t)blockIdx.x * ADAM_BLOCK + threadIdx.x;
  const bool actor = i < L.total && is_actor_element(L, i);
  const int64_t il = actor ? i : L.p_w1;   // the loads go out before the norm is known; threads without an element read a valid one
  const float g_in = g[il], m_in = m[il], v_in = v[il], p_in = p[il];
  double s = 0.0;
  if (threadIdx.x < 64) s = norm_partials_sum(partials, n_partials);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);
    const int st = (host_step > 0 ? host_step : step_dev[CNT_STEP]) + step_dev[CNT_EXTRA] + 1;
    sh[0] = max_norm > 0.f ? fminf(max_norm / (norm + 1e-6f), 1.f) : 1.f;
    if (step_dev[AREC_ST] == st) {   // anchor_finalize_kernel left the corrections of this count (uniform branch)
      sh[1] = (float)((double)lr / *reinterpret_cast<const double*>(step_dev + AREC_BC1));
      sh[2] = __int_as_float(step_dev[AREC_BC2]);
    } else {   // a step count given by the caller that is not the device's
      sh[1] = (float)((double)lr / anchor_bias1(st));
      sh[2] = anchor_bias2_sqrt(st);
    }
  }
  __syncthreads();
  if (actor) {
    const float gi = g_in * sh[0];
    const float mn = 0.9f * m_in + 0.1f * gi;
    const float vn = 0.999f * v_in + 0.001f * gi * gi;
    const float denom = sqrtf(vn) / sh[2] + eps;
    const float pn = p_in - sh[1] * (mn / denom);
    m[i] = mn; v[i] = vn; p[i] = pn;
    pack_one(i, pn, L, k);
  }
}

// the actor tensors have taken one more step than the rest: a launch of its own, after every block of anchor_adam_kernel has read the count
#ifndef KP1_MLP_LINE_TU
__global__ void anchor_count_kernel(int* __restrict__ cnt) {
  const int extra = cnt[CNT_EXTRA] + 1;
  cnt[CNT_EXTRA] = extra;
  adam_record_write(cnt, cnt[CNT_STEP], extra);   // an Adam launch on the device's counts finds its corrections whichever launch came last
}
#endif

#include "kp1_env_step.inc"
#include "kp1_eval_step.inc"
#include "kp1_rollout_step.inc"
#include "kp1_mlp_tile.inc"
#ifdef KP1_MLP_LINE_TU
// kp1_mlp_line.hip includes this file for the text above and nothing else: it instantiates the kernels only a handle with a hyper-parameter
// line launches in a code object of its own, so that this file's code object is not touched by them
}  // namespace
#else
#include "kp1_mlp_fused.inc"
// (new kernels go after the tile kernels: including them earlier moved the tile kernels' addresses)
#include "kp1_route_step.inc"
#include "kp1_route_rollout_step.inc"
#include "kp1_route_chain_step.inc"
#include "kp1_rollout_run.inc"       // behind every kernel of its parent: each of those keeps its place in the code object
#include "kp1_train_tile.inc"        // last, for the same reason

}  // namespace

#include "kp1_route_host.hpp"

// ============================================================================================ host
struct kp1_mlp {
  int device = 0, H = 0, Hp = 0, max_batch = 0;
  // Population handle (kp1_mlp_create_population): K independent replicas of the layer-wise (Hp = 128) path, launched together with the
  // replica on a grid axis.  Every array below except xf and step_dev holds K copies back to back (replica r at + r * its per-replica size).
  int K = 1;
  ParamLayout L;
  Packed k{};
  float* h1 = nullptr;   // [2][max_batch][Hp]
  float* h2 = nullptr;
  float* dz2 = nullptr;
  float* dz1 = nullptr;
  float* xf = nullptr;    // [max_batch][64] gathered observations, k8-fragment major (fused path)
  // [r3 experiment, KP1_MLP_OPT_BF16X3_WGRAD] the same four tensors as three bf16 planes each, allocated when the option is first switched on
  int bf16x3 = 0;
  unsigned short* sp_h1 = nullptr; unsigned short* sp_dz2 = nullptr; unsigned short* sp_dz1 = nullptr; unsigned short* sp_xf = nullptr;
  double* partials = nullptr;  // [512]
  double* anchor_partials = nullptr;   // [K][ANCHOR_PARTIALS] sum-of-squares partials of kp1_mlp_anchor_loss_grad (Hp = 128 handles)
  float* slab = nullptr;       // [64 chunks][2 nets][Hp][Hp] partial dW2
  float* slab1 = nullptr;      // [64 chunks][2 nets][Hp][64] partial dW1
  float* bslab = nullptr;      // [max_batch/64 row tiles][2 nets][Hp] partial db1
  float* hpart = nullptr;      // [max_batch/32 blocks][10 Hp + 32] head partials
  int n_finalize_blocks = 0;   // sum-of-squares partials written by the last grad_finalize_kernel
  int* step_dev = nullptr;     // device Adam step counts and the record of their bias corrections (CNT_*, REC_*, AREC_*): K lines, line 0 the shared one
  // KL early stop (kp1_mlp_set_kl_gate): one record per replica; while gate_on, finalize and Adam run their gated forms on line r of step_dev
  kp1_kl_gate* gate_dev = nullptr;
  bool gate_on = false;
  int actor_extra_host = 0;    // host mirror of [CNT_EXTRA] (set_option + one per anchor Adam step): a gate refuses a non-zero one
  // hyper-parameter table [K][HP_FIELDS] (kp1_mlp_set_replica_hparams; kp1_mlp_hparams_store, which also gives a K = 1 handle its one
  // line); the kernels read it while hparams_on -- a K = 1 handle then launches the forms that read it (line_on below)
  float* hparams_dev = nullptr;
  bool hparams_on = false;
  int last_s2_n = 0, last_s1_n = 0;
  int train_tile = 0;          // KP1_MLP_OPT_TRAIN_TILE: kp1_mlp_loss_grad of an Hp = 128 handle in one tile launch (train_tile128_kernel)
  int fused = 1;               // KP1_MLP_OPT_FUSED: one workgroup carries a row tile through the whole chain (H = 256 only)
  // While the fused path is selected the Adam kernel refreshes only the fragment-major weight copies (the transposed / slab copies are
  // scattered 4-byte writes and were half of the kernel's HBM write traffic); the k-slab copies are then stale until the next full pack, which switching the
  // option off triggers from the parameter vector last seen.
  const float* last_params = nullptr;
  bool slab_stale = false;
  std::vector<void*> allocs;
  // KP1_MLP_OPT_PROFILE: a HIP-event pair attached to every launch of the optimiser step (hipExtLaunchKernelGGL: the dispatch's own begin
  // and end), on the launch stream, in the real launch sequence (tile -> weight gradients -> finalize -> Adam), read back by
  // kp1_mlp_profile_read.  Off in production (an eager epoch: events do not travel into a captured graph replay).
  int profile = 0;
  struct ProfPair { hipEvent_t a, b; };
  std::vector<ProfPair> prof[KP1_MLP_PROFILE_SLOTS];
  int prof_used[KP1_MLP_PROFILE_SLOTS] = {0, 0, 0, 0};
};

namespace {
// The event pair of the profiled launch in flight on this thread.  KP1_LAUNCH hands it to hipExtLaunchKernelGGL, which attaches both events
// to the kernel's own dispatch packet: their elapsed time is the dispatch's begin -> end, the interval rocprofv3 --kernel-trace reports.
// (Round 2 recorded the events as separate stream markers around the launch; that interval also holds the marker -> dispatch hand-over,
// 2-4 us on this stack, and read 50.6 us where rocprofv3 read 48.5 for the same launches.)  A scope whose launch site does not use
// KP1_LAUNCH falls back to the marker pair.
struct ProfSlotInFlight { hipEvent_t a = nullptr, b = nullptr; bool attached = false; };
thread_local ProfSlotInFlight tl_prof;

struct ProfScope {
  kp1_mlp* m; int slot; hipStream_t stream; bool on;
  ProfScope(kp1_mlp* m_, int slot_, hipStream_t s_) : m(m_), slot(slot_), stream(s_), on(m_->profile != 0) {
    if (!on) return;
    auto& v = m->prof[slot];
    if (m->prof_used[slot] >= (int)v.size()) {
      kp1_mlp::ProfPair p{};
      if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) { on = false; return; }
      v.push_back(p);
    }
    tl_prof.a = v[m->prof_used[slot]].a;
    tl_prof.b = v[m->prof_used[slot]].b;
    tl_prof.attached = false;
  }
  ~ProfScope() {
    if (!on) return;
    if (!tl_prof.attached) {   // nothing was launched through KP1_LAUNCH inside the scope: an empty marker pair (reads ~0)
      (void)hipEventRecord(tl_prof.a, stream);
      (void)hipEventRecord(tl_prof.b, stream);
    }
    tl_prof = ProfSlotInFlight{};
    m->prof_used[slot] += 1;
  }
};

// launch of a kernel that may be inside a ProfScope
#define KP1_LAUNCH(kernel, grid, block, bytes, stream, ...)                                                        \
  do {                                                                                                             \
    if (tl_prof.a != nullptr && !tl_prof.attached) {                                                               \
      tl_prof.attached = true;                                                                                     \
      hipExtLaunchKernelGGL(kernel, grid, block, bytes, stream, tl_prof.a, tl_prof.b, 0, __VA_ARGS__);             \
    } else {                                                                                                       \
      hipLaunchKernelGGL(kernel, grid, block, bytes, stream, __VA_ARGS__);                                         \
    }                                                                                                              \
  } while (0)
}  // namespace

namespace {

constexpr int N_PARTIALS = 128;
constexpr int ANCHOR_PARTIALS = 256;   // blocks of anchor_finalize_kernel: 256 parameters each, 215 for the largest layer-wise net (2x128, 80 inputs)
constexpr int PARTIALS_STRIDE = 2 * N_PARTIALS + 2048;   // doubles of kp1_mlp::partials per replica
// batch chunks of the dW2 / dW1 partial tiles of gemm_tn_split_kernel: 8 chunks x 32 tiles = one dW2 workgroup per CU, 16 chunks x 16 tiles of
// quarter-size dW1 workgroups (profiles/r02_ab_tn_wave_split.log)
constexpr int TN_SPLIT2 = 8, TN_SPLIT1 = 16;

// rows of the batch each TN workgroup reduces: aim at ~256 workgroups (one per CU) for the H x H gradient
int tn_chunk_rows(int n, int tiles) {
  int chunks = (256 + tiles - 1) / tiles;
  if (chunks > 64) chunks = 64;     // slab capacity (kp1_mlp_create)
  if (chunks < 1) chunks = 1;
  int rows = (n + chunks - 1) / chunks;
  rows = (rows + 63) / 64 * 64;     // whole 64-row stages
  return rows < 64 ? 64 : rows;
}

int mlp_check_device(const kp1_mlp* m) {
  HIP_TRY(hipSetDevice(m->device));
  return KP1_OK;
}

// ---- argument builders: each block of kernel arguments that more than one entry point fills is filled here, once

// the n / obs_stride checks that open kp1_mlp_forward, kp1_mlp_loss_grad and kp1_mlp_anchor_loss_grad
int check_batch_args(const kp1_mlp* m, int n, int obs_stride) {
  if (n <= 0 || n > m->max_batch) return fail(KP1_ERR_INVALID, "n exceeds the workspace max_batch");
  if (obs_stride != m->L.IN && obs_stride != m->L.INP)
    return fail(KP1_ERR_INVALID, "obs_stride must be the observation width or its padded width (56 / 64, or 80 / 128)");
  return KP1_OK;
}

// floats of an observation row that layer 1 loads: the padded width when the rows are stored padded, else the real one
int kreal(const kp1_mlp* m, int obs_stride) {
  const int IN = m->L.IN, INP = m->L.INP;
  return obs_stride >= INP ? INP : IN;
}

// FusedArgs: the observation rows and the weights, common to every form of the tile kernel
void fill_fused_head(FusedArgs& fa, const kp1_mlp* m, const float* obs, int obs_stride, const int64_t* idx, int n) {
  fa.obs = obs; fa.obs_stride = obs_stride; fa.Kreal = kreal(m, obs_stride); fa.inp = m->L.INP; fa.idx = idx; fa.n = n;
  fa.k = m->k;
}

// weights, biases and per-replica strides of a layer-wise argument block (net 0, the policy, leads every array).  EvalStepArgs runs the policy
// net only and the mean action: it has no per-net strides and no log_std.
template <class Args>
void fill_layer_weights(Args& a, const kp1_mlp* m) {
  const int Hp = m->Hp, INP = m->L.INP;
  a.w1 = m->k.w1p; a.b1 = m->k.b1; a.w2 = m->k.w2; a.b2 = m->k.b2; a.w3 = m->k.w3; a.b3 = m->k.b3;
  a.r_w1 = (unsigned)(2 * Hp * INP); a.r_w2 = (unsigned)(2 * Hp * Hp); a.r_b = (unsigned)(2 * Hp); a.r_w3 = (unsigned)(HEADS * Hp); a.r_b3 = (unsigned)HEADS;
  if constexpr (std::is_same_v<Args, RolloutStepArgs>) {
    a.log_std = m->k.log_std;
    a.n_w1 = (unsigned)(Hp * INP); a.n_w2 = (unsigned)(Hp * Hp); a.n_b = (unsigned)Hp;
  }
}

// the forward half of a RolloutStepArgs (its env block is the caller's): n rows per replica
void fill_rollout_forward(RolloutStepArgs& f, const kp1_mlp* m, const float* obs, int obs_stride, const float* noise, float* value, float* action,
                          float* log_prob, int n) {
  f.obs = obs; f.obs_stride = obs_stride;
  fill_layer_weights(f, m);
  f.noise = noise; f.value = value; f.action = action; f.log_prob = log_prob;
  f.n = n;
  f.Kreal = kreal(m, obs_stride);
}

// dZ1 = (dZ2 W2) * (1 - h1^2), bias-1 gradient partials = per-row-tile column sums of dZ1 (launch_nt<EPI_DTANH>)
GemmNT backward_nt_args(const kp1_mlp* m, int n) {
  const int Hp = m->Hp;
  const int64_t act_stride = (int64_t)m->max_batch * Hp;
  GemmNT g{};
  g.A = m->dz2; g.lda = Hp; g.strideA = act_stride; g.gather = nullptr;
  g.W = m->k.w2t; g.strideW = (int64_t)Hp * Hp;
  g.bias = nullptr; g.strideBias = 0;
  g.C = m->dz1; g.ldc = Hp; g.strideC = act_stride;
  g.aux = m->h1; g.strideAux = act_stride;
  g.colsum = m->bslab; g.strideColsum = Hp;
  g.M = n; g.N = Hp; g.K = Hp; g.Kreal = Hp;
  g.reps = m->K;
  g.r_A = g.r_C = g.r_aux = (unsigned)(2 * act_stride); g.r_W = (unsigned)(2 * Hp * Hp);
  g.r_colsum = (unsigned)((m->max_batch / 32) * 2 * Hp);
  return g;
}

// weight gradients of the tile path: the dW2 / dW1 slabs and the batch chunking of gemm_tn_split_kernel (and of its bf16x3 form)
TnFragArgs tn_frag_args(const kp1_mlp* m, int n) {
  const int Hp = m->Hp, INP = m->L.INP;
  TnFragArgs t{};
  t.inp = INP;
  t.dz2 = m->dz2; t.h1 = m->h1; t.dz1 = m->dz1; t.act_stride = (int64_t)m->max_batch * Hp; t.xf = m->xf;
  t.slab2 = m->slab; t.s2_net = (int64_t)Hp * Hp; t.s2_chunk = 2 * t.s2_net;
  t.slab1 = m->slab1; t.s1_net = (int64_t)Hp * INP; t.s1_chunk = 2 * t.s1_net;
  t.groups = (n + FU_BM - 1) / FU_BM * (FU_BM / 8);   // the tile kernel writes whole 32-row tiles
  auto up8 = [](int v) { return (v + 7) / 8 * 8; };
  t.cg2 = up8((t.groups + TN_SPLIT2 - 1) / TN_SPLIT2);
  t.cg1 = up8((t.groups + TN_SPLIT1 - 1) / TN_SPLIT1);
  t.n_chunks2 = (t.groups + t.cg2 - 1) / t.cg2;
  t.n_chunks1 = (t.groups + t.cg1 - 1) / t.cg1;
  return t;
}

// number of row tiles launch_nt uses for an n-row GEMM with N = Hp columns (the bias-partial count of the backward GEMM)
int nt_row_tiles(int n, int Hp) {
  (void)Hp;
  return (n + 63) / 64;
}

// FinalizeArgs: where the gradient's parts lie (slabs, bias and head partials, per-replica strides) after an n-row backward pass with s2_n / s1_n
// batch chunks.  b_n is the layer-wise row-tile count; the loss terms, the outputs and the sum-of-squares buffer are the caller's.
void fill_finalize(FinalizeArgs& f, const kp1_mlp* m, int n, int s2_n, int s1_n, float* grad) {
  const int Hp = m->Hp, INP = m->L.INP;
  f.L = m->L;
  f.slab2 = m->slab; f.s2_ld = Hp; f.s2_net = (int64_t)Hp * Hp; f.s2_chunk = 2 * f.s2_net; f.s2_n = s2_n;
  f.slab1 = m->slab1; f.s1_ld = INP; f.s1_net = (int64_t)Hp * INP; f.s1_chunk = 2 * f.s1_net; f.s1_n = s1_n;
  f.bslab = m->bslab; f.b_net = Hp; f.b_tile = 2 * Hp; f.b_n = nt_row_tiles(n, Hp);
  f.hpart = m->hpart; f.h_stride = 10 * Hp + 32; f.h_n = (n + HEAD_ROWS - 1) / HEAD_ROWS;
  f.log_std = m->k.log_std;
  f.grad = grad;
  f.r_slab2 = (unsigned)(64 * f.s2_chunk); f.r_slab1 = (unsigned)(64 * f.s1_chunk); f.r_bslab = (unsigned)((m->max_batch / 32) * 2 * Hp);
  f.r_hpart = (unsigned)((int64_t)(m->max_batch / 32) * (10 * Hp + 32));
}

constexpr size_t TN_LDS_BYTES = sizeof(float) * 2 * 2 * 64 * (128 + 4);

// Tile shapes.  Wide (whole hidden width per workgroup, large batches): 64 rows x 256 columns, 32-deep W stages, 512
// threads (two waves per SIMD split the epilogue), one workgroup per CU.  Narrow (small batches, more workgroups):
// 64 rows x 128 columns, 256 threads.  Measured alternatives at M = 8192 (all within 7 %): 32 x 256 tiles with 16-deep
// stages and two workgroups per CU 29.9 us, 64 x 256 / 256 threads 28.9 us, this one 28.0 us -- the three GEMM kinds all
// plateau near 75 TFLOP/s, see DESIGN.md section 5.
template <int BN, int EPI, int K, bool POP = false>
int launch_nt_inst(const GemmNT& g, hipStream_t stream) {
  constexpr int NTH = BN == 256 ? 512 : 256;
  constexpr int BM = 64;
  constexpr int BKS = 32;
  size_t bytes = sizeof(float) * (BM * (size_t)(K + 4) + 2 * (size_t)BN * (BKS + 4));
  const size_t epi = sizeof(float) * (BM * (size_t)(BN + 4) + (size_t)(NTH / (BN / 4)) * BN);  // C tile + bias-partial scratch
  if (epi > bytes) bytes = epi;
  HIP_TRY(hipFuncSetAttribute((const void*)gemm_nt_kernel<BN, EPI, K, NTH, BM, BKS, POP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  hipLaunchKernelGGL((gemm_nt_kernel<BN, EPI, K, NTH, BM, BKS, POP>), dim3((g.M + BM - 1) / BM, g.N / BN, POP ? 2 * g.reps : 2), dim3(NTH), bytes, stream, g);
  return KP1_OK;
}

template <int EPI>
int launch_nt(const GemmNT& g, hipStream_t stream) {
  if (g.N % 128 != 0) return fail(KP1_ERR_INVALID, "gemm_nt needs N % 128 == 0");
  if (g.reps > 1) {   // population handles: Hp = 128 (narrow tiles, as a single handle of that width uses); K = INP (64 / 128) or Hp
    if (g.N != 128) return fail(KP1_ERR_UNSUPPORTED, "population gemm_nt is instantiated for N = 128");
    if (g.K == 64) return launch_nt_inst<128, EPI, 64, true>(g, stream);
    if (g.K == 128) return launch_nt_inst<128, EPI, 128, true>(g, stream);
    return fail(KP1_ERR_UNSUPPORTED, "population gemm_nt is instantiated for K in {64, 128}");
  }
  // 256-column workgroups (A read once per row block) when that still fills the chip, else 128-column ones
  const int row_tiles = (g.M + 63) / 64;
  const bool wide = (g.N % 256 == 0) && row_tiles * 2 >= 200;
  if (g.K == 64) return wide ? launch_nt_inst<256, EPI, 64>(g, stream) : launch_nt_inst<128, EPI, 64>(g, stream);
  if (g.K == 128) return wide ? launch_nt_inst<256, EPI, 128>(g, stream) : launch_nt_inst<128, EPI, 128>(g, stream);
  if (g.K == 256) return wide ? launch_nt_inst<256, EPI, 256>(g, stream) : launch_nt_inst<128, EPI, 256>(g, stream);
  return fail(KP1_ERR_UNSUPPORTED, "gemm_nt is instantiated for K in {64, 128, 256}");
}

// dW (both nets) = D^T X over n rows: split-B partial tiles into m->slab, then the fixed-order reduce into G
int launch_tn(kp1_mlp* m, GemmTN t, int n_o_tiles, int slab_cols, float* slab, int* n_chunks_out, hipStream_t stream);

// Every launch of mlp_tile_kernel: the dynamic-LDS attribute, then the launch.  Only the training forms go through KP1_LAUNCH: they are the ones
// the optimiser step's profile covers.
template <bool TRAIN, int K1S, int ENV = 0, bool SPLIT = false>
int launch_tile(dim3 grid, const FusedArgs& fa, hipStream_t stream) {
  const size_t bytes = sizeof(float) * FU_LDS_FLOATS;   // 32-row tiles, 4 waves
  HIP_TRY(hipFuncSetAttribute((const void*)mlp_tile_kernel<TRAIN, K1S, ENV, SPLIT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  if constexpr (TRAIN) KP1_LAUNCH((mlp_tile_kernel<TRAIN, K1S, ENV, SPLIT>), grid, dim3(FU_NTH), bytes, stream, fa);
  else hipLaunchKernelGGL((mlp_tile_kernel<TRAIN, K1S, ENV, SPLIT>), grid, dim3(FU_NTH), bytes, stream, fa);
  return KP1_OK;
}

// the training tile's grid, and the hold-back of the second workgroup of every CU
dim3 fused_train_shape(FusedArgs& fa) {
  static const int stagger_us = [] { const char* e = std::getenv("KP1_FU_STAGGER_US"); return e ? std::atoi(e) : 11; }();  // tuning knob; re-swept in round 3 (profiles/r03_ab_tile_stagger.log): 10-13 us within 0.4 us of each other, a cliff at 14 (+6 us)
  static const int n_cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 256;
    return n;
  }();
  const dim3 grid((fa.n + FU_BM - 1) / FU_BM, 1, 2);
  fa.n_cus = n_cus;
  fa.stagger_ticks = (int)(grid.x * grid.z) > n_cus ? stagger_us * 100 : 0;   // only when CUs hold two workgroups at once
  return grid;
}

int launch_fused(const FusedArgs& fa_in, hipStream_t stream) {
  FusedArgs fa = fa_in;
  const dim3 grid = fused_train_shape(fa);
  if (fa.sp_h1 != nullptr)   // [r3 experiment] bf16 x 3 planes instead of the fp32 activation copies
    return fa.inp == 64 ? launch_tile<true, 2, 0, true>(grid, fa, stream) : launch_tile<true, 4, 0, true>(grid, fa, stream);
  return fa.inp == 64 ? launch_tile<true, 2>(grid, fa, stream) : launch_tile<true, 4>(grid, fa, stream);
}

// policy forward + env step in one launch (kp1_mlp_forward_env_step): env_mode = KP1_MODE_APPROACH / KP1_MODE_DOCK, 64-float observation rows
int launch_fused_infer_env(const FusedArgs& fa, int env_mode, hipStream_t stream) {
  const dim3 grid((fa.n + FU_BM - 1) / FU_BM, 1, fa.value ? 2 : 1);
  return env_mode == KP1_MODE_DOCK ? launch_tile<false, 2, 2>(grid, fa, stream) : launch_tile<false, 2, 1>(grid, fa, stream);
}

// deterministic evaluation step of a 2x256 policy in one launch (kp1_eval_step): policy net only, the bookkeeping of fa.ev in the tail
int launch_fused_eval_env(const FusedArgs& fa, int env_mode, hipStream_t stream) {
  const dim3 grid((fa.n + FU_BM - 1) / FU_BM, 1, 1);
  return env_mode == KP1_MODE_DOCK ? launch_tile<false, 2, 4>(grid, fa, stream) : launch_tile<false, 2, 3>(grid, fa, stream);
}

// whole-episode evaluation of a 2x256 policy in one launch (kp1_eval_episodes): env steps fa.ev.step .. fa.ev.last_step, one workgroup per tile
int launch_fused_eval_episodes(const FusedArgs& fa, int env_mode, hipStream_t stream) {
  const dim3 grid((fa.n + FU_BM - 1) / FU_BM, 1, 1);
  return env_mode == KP1_MODE_DOCK ? launch_tile<false, 2, 6>(grid, fa, stream) : launch_tile<false, 2, 5>(grid, fa, stream);
}

int launch_fused_infer(const FusedArgs& fa, hipStream_t stream) {
  // the value net is skipped when no value is asked for (deterministic evaluators), the policy net when only values are
  const bool want_pi = fa.mean || fa.action || fa.clipped || fa.log_prob;
  if (!want_pi && !fa.value) return KP1_OK;
  FusedArgs f = fa;
  const bool both = want_pi && fa.value;
  if (!both) f.net_base = want_pi ? 0 : 1;
  const dim3 grid((fa.n + FU_BM - 1) / FU_BM, 1, both ? 2 : 1);
  return fa.inp == 64 ? launch_tile<false, 2>(grid, f, stream) : launch_tile<false, 4>(grid, f, stream);
}

int launch_tn_frag(const TnFragArgs& t, hipStream_t stream) {
  if (t.n_chunks2 > 64 || t.n_chunks1 > 64) return fail(KP1_ERR_INVALID, "too many batch chunks for the partial-gradient slabs");
  const size_t bytes = sizeof(float) * TN_SPLIT_LDS_FLOATS;
  HIP_TRY(hipFuncSetAttribute((const void*)gemm_tn_split_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  KP1_LAUNCH(gemm_tn_split_kernel, dim3(32 * t.n_chunks2 + 16 * t.n_chunks1), dim3(256), bytes, stream, t);
  return KP1_OK;
}

// forward layers 1 and 2 for n rows (both nets): h1, h2 filled
// (population: n rows per replica; without idx replica r reads obs rows [r n, (r + 1) n), with idx its index row idx[r][0..n))
int launch_forward_layers(kp1_mlp* m, const float* obs, int obs_stride, const int64_t* idx, int n, hipStream_t stream) {
  const int Hp = m->Hp, INP = m->L.INP;
  const int64_t act_stride = (int64_t)m->max_batch * Hp;
  GemmNT g{};
  g.reps = m->K;
  g.r_A = idx ? 0u : (unsigned)(n * obs_stride); g.r_gather = (unsigned)n;
  g.r_W = (unsigned)(2 * Hp * INP); g.r_bias = (unsigned)(2 * Hp); g.r_C = (unsigned)(2 * act_stride);
  g.A = obs; g.lda = obs_stride; g.strideA = 0; g.gather = idx;
  g.W = m->k.w1p; g.strideW = (int64_t)Hp * INP;
  g.bias = m->k.b1; g.strideBias = Hp;
  g.C = m->h1; g.ldc = Hp; g.strideC = act_stride;
  g.aux = nullptr; g.strideAux = 0; g.colsum = nullptr; g.strideColsum = 0;
  g.M = n; g.N = Hp; g.K = INP; g.Kreal = kreal(m, obs_stride);
  int rc = launch_nt<EPI_BIAS_TANH>(g, stream);
  if (rc != KP1_OK) return rc;
  g.A = m->h1; g.lda = Hp; g.strideA = act_stride; g.gather = nullptr;
  g.r_A = (unsigned)(2 * act_stride); g.r_W = (unsigned)(2 * Hp * Hp);
  g.W = m->k.w2; g.strideW = (int64_t)Hp * Hp;
  g.bias = m->k.b2;
  g.C = m->h2;
  g.K = Hp; g.Kreal = Hp;
  rc = launch_nt<EPI_BIAS_TANH>(g, stream);
  if (rc != KP1_OK) return rc;
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}

}  // namespace

namespace {
int launch_tn(kp1_mlp* m, GemmTN t, int n_o_tiles, int slab_cols, float* slab, int* n_chunks_out, hipStream_t stream) {
  const int Hp = m->Hp;
  const int n_chunks = (t.B + t.chunk - 1) / t.chunk;
  if (n_chunks > 64) return fail(KP1_ERR_INVALID, "too many batch chunks for the partial-gradient slab");
  t.slab = slab;
  t.slab_ld = slab_cols;
  t.slab_net_stride = (int64_t)Hp * slab_cols;
  t.slab_chunk_stride = 2 * t.slab_net_stride;
  const dim3 grid(n_chunks, n_o_tiles * t.n_i_tiles, 2 * m->K);
  if (m->K > 1) {   // population: replica r's activations at + r * 2 act_stride, its gather row at + r * B, its slab at + r * 64 chunks
    t.reps = m->K;
    t.r_D = (unsigned)(2 * (int64_t)m->max_batch * Hp);
    t.r_X = t.gatherX ? 0u : t.r_D;
    t.r_gather = (unsigned)t.B;
    t.r_slab = (unsigned)(64 * t.slab_chunk_stride);
  }
  const bool gather = t.gatherX != nullptr;
  // the four gemm_tn_kernel instantiations share the LDS size
  auto* kernel = m->K > 1 ? (gather ? gemm_tn_kernel<true, true> : gemm_tn_kernel<false, true>) : (gather ? gemm_tn_kernel<true> : gemm_tn_kernel<false>);
  HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TN_LDS_BYTES));
  hipLaunchKernelGGL(kernel, grid, dim3(256), TN_LDS_BYTES, stream, t);
  if (n_chunks_out) *n_chunks_out = n_chunks;
  return KP1_OK;
}

// weight gradients of the layer-wise path (split over the batch axis): the dW2 and dW1 slabs of an n-row backward pass, *s2_n / *s1_n chunks
int launch_layer_wgrads(kp1_mlp* m, const float* obs, int obs_stride, const int64_t* idx, int n, int* s2_n, int* s1_n, hipStream_t stream) {
  const int Hp = m->Hp;
  const int64_t act_stride = (int64_t)m->max_batch * Hp;
  GemmTN t{};
  t.B = n;
  t.chunk = tn_chunk_rows(n, (Hp / 128) * (Hp / 128) * 2);
  // dW2[o][i] = sum_b dZ2[b][o] h1[b][i]
  t.D = m->dz2; t.ldd = Hp; t.strideD = act_stride;
  t.X = m->h1; t.ldx = Hp; t.strideX = act_stride; t.gatherX = nullptr;
  t.Nload = Hp; t.n_i_tiles = Hp / 128;
  int rc = launch_tn(m, t, Hp / 128, Hp, m->slab, s2_n, stream);
  if (rc != KP1_OK) return rc;
  // dW1[o][i] = sum_b dZ1[b][o] x[b][i]   (i < 56)
  t.D = m->dz1;
  t.X = obs; t.ldx = obs_stride; t.strideX = 0; t.gatherX = idx;
  t.Nload = kreal(m, obs_stride); t.n_i_tiles = 1;
  t.chunk = tn_chunk_rows(n, (Hp / 128) * 2);  // few tiles: more, shorter batch chunks keep the CUs busy
  return launch_tn(m, t, Hp / 128, m->L.INP, m->slab1, s1_n, stream);
}

// KP1_MLP_OPT_TRAIN_TILE (defined at the end of this file, see there)
int launch_train_tile(kp1_mlp* m, const HeadArgs& heads, const float* obs, int obs_stride, int chunks, float* grad, hipStream_t stream);
// the training tile of a K = 1 hidden-256 handle with a hyper-parameter line (kp1_mlp_hparams_store): the launch is kp1_mlp_line.hip's
int launch_fused_line(const FusedArgs& fa_in, const float* line, hipStream_t stream) {
  FusedArgs fa = fa_in;
  const dim3 grid = fused_train_shape(fa);
  hipEvent_t start = nullptr, stop = nullptr;   // KP1_LAUNCH's profile events, handed across
  if (tl_prof.a != nullptr && !tl_prof.attached) {
    tl_prof.attached = true;
    start = tl_prof.a; stop = tl_prof.b;
  }
  return kp1::mlp_line_launch_tile(&fa, sizeof(fa), line, grid, start, stop, stream);
}
}  // namespace

extern "C" {

int64_t kp1_mlp_num_params(int32_t hidden) { return hidden > 0 ? make_layout(hidden).total : 0; }
int64_t kp1_mlp_num_params_ex(int32_t hidden, int32_t obs_dim) { return hidden > 0 && obs_dim > 0 && obs_dim <= 128 ? make_layout(hidden, obs_dim).total : 0; }

int kp1_mlp_create(int32_t device, int32_t hidden, int32_t max_batch, kp1_mlp** out) { return kp1_mlp_create_ex(device, hidden, KP1_MLP_IN, max_batch, out); }

namespace {
int mlp_create(int32_t device, int32_t hidden, int32_t obs_dim, int32_t max_batch, int32_t replicas, kp1_mlp** out);
}

int kp1_mlp_create_ex(int32_t device, int32_t hidden, int32_t obs_dim, int32_t max_batch, kp1_mlp** out) {
  return mlp_create(device, hidden, obs_dim, max_batch, 1, out);
}

int kp1_mlp_create_population(int32_t device, int32_t hidden, int32_t obs_dim, int32_t max_batch, int32_t replicas, kp1_mlp** out) {
  if (replicas < 1 || replicas > KP1_MLP_MAX_REPLICAS) return fail(KP1_ERR_INVALID, "replicas must be in [1, KP1_MLP_MAX_REPLICAS]");
  if (hidden != 64 && hidden != 128)
    return fail(KP1_ERR_UNSUPPORTED, "population handles run the layer-wise kernels: hidden must be 64 or 128");
  if (obs_dim != KP1_MLP_IN && obs_dim != KP1_MLP_IN_ROUTE)
    return fail(KP1_ERR_UNSUPPORTED, "population handles take the 56-float or the 80-float (route) observation");
  // per-replica element offsets are 32-bit: the largest arrays (the dW2 / dW1 partial slabs, 64 chunks x 2 nets x 128 x INP with INP <= 128)
  // and the activations of K replicas must stay below 2^31 elements
  const int64_t mb = ((int64_t)max_batch + 127) / 128 * 128;
  if (max_batch <= 0 || (int64_t)replicas * 2 * mb * 128 >= ((int64_t)1 << 31)) return fail(KP1_ERR_INVALID, "max_batch too large for a population handle");
  return mlp_create(device, hidden, obs_dim, max_batch, replicas, out);
}

int32_t kp1_mlp_replicas(const kp1_mlp* m) { return m ? m->K : 0; }

}  // extern "C"

namespace {
int mlp_create(int32_t device, int32_t hidden, int32_t obs_dim, int32_t max_batch, int32_t replicas, kp1_mlp** out) {
  if (!out || hidden <= 0 || hidden > 1024 || max_batch <= 0) return fail(KP1_ERR_INVALID, "bad argument to kp1_mlp_create");
  if (obs_dim != KP1_MLP_IN && obs_dim != KP1_MLP_IN_ROUTE)
    return fail(KP1_ERR_UNSUPPORTED, "obs_dim must be 56 (ArmKinematicEnv) or 80 (route observation keys)");
  // 256: the fused tile path (BASELINE config 2).  128 and 64 (SB3's default net_arch, what the reference trains and what its checkpoints
  // hold): the layer-wise MFMA kernels on a 128-wide padded layout -- padded hidden units have zero weights and biases, so they stay at
  // tanh(0) = 0 in the forward pass and receive exactly zero gradient; finalize / Adam / the gradient norm only ever touch the H real rows.
  if (hidden != 64 && hidden != 128 && hidden != 256)
    return fail(KP1_ERR_UNSUPPORTED, "hidden must be 64 (SB3 default), 128 or 256 (the widths the MFMA kernels are instantiated for)");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(KP1_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
  if (device < 0 || device >= count) return fail(KP1_ERR_INVALID, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  kp1_mlp* m = new kp1_mlp();
  m->device = device;
  m->K = replicas;
  m->H = hidden;
  m->L = make_layout(hidden, obs_dim);
  m->Hp = m->L.Hp;
  m->max_batch = (max_batch + 127) / 128 * 128;
  const int64_t Hp = m->Hp, mb = m->max_batch, INP = m->L.INP, K = m->K;
  auto alloc = [&](void** p, size_t bytes) -> int {
    if (hipMalloc(p, bytes) != hipSuccess) return fail(KP1_ERR_ALLOC, "hipMalloc failed in kp1_mlp_create");
    m->allocs.push_back(*p);
    return hipMemset(*p, 0, bytes) == hipSuccess ? KP1_OK : fail(KP1_ERR_NO_DEVICE, "hipMemset failed");
  };
  int rc = KP1_OK;
#define MLP_ALLOC(ptr, count) if (rc == KP1_OK) rc = alloc((void**)&(ptr), sizeof(*(ptr)) * (size_t)(count))
  MLP_ALLOC(m->k.w1p, K * 2 * Hp * INP);
  MLP_ALLOC(m->k.b1, K * 2 * Hp);
  MLP_ALLOC(m->k.w2, K * 2 * Hp * Hp);
  MLP_ALLOC(m->k.w2t, K * 2 * Hp * Hp);
  MLP_ALLOC(m->k.w1f, K * 2 * Hp * INP);
  MLP_ALLOC(m->k.w2f, K * 2 * Hp * Hp);
  MLP_ALLOC(m->k.w2tf, K * 2 * Hp * Hp);
  MLP_ALLOC(m->k.b2, K * 2 * Hp);
  MLP_ALLOC(m->k.w3, K * HEADS * Hp);
  MLP_ALLOC(m->k.b3, K * HEADS);
  MLP_ALLOC(m->k.log_std, K * HEADS);
  MLP_ALLOC(m->h1, K * 2 * mb * Hp);
  MLP_ALLOC(m->h2, K * 2 * mb * Hp);
  MLP_ALLOC(m->dz2, K * 2 * mb * Hp);
  MLP_ALLOC(m->dz1, K * 2 * mb * Hp);
  MLP_ALLOC(m->xf, mb * INP);
  MLP_ALLOC(m->partials, K * PARTIALS_STRIDE);
  if (Hp == 128) MLP_ALLOC(m->anchor_partials, K * ANCHOR_PARTIALS);
  MLP_ALLOC(m->slab, K * 64 * 2 * Hp * Hp);
  MLP_ALLOC(m->slab1, K * 64 * 2 * Hp * INP);
  MLP_ALLOC(m->step_dev, K * STEP_DEV_INTS);
  MLP_ALLOC(m->gate_dev, K);
  if (K > 1) MLP_ALLOC(m->hparams_dev, K * HP_FIELDS);
  MLP_ALLOC(m->bslab, K * (mb / 32) * 2 * Hp);
  MLP_ALLOC(m->hpart, K * (mb / 32) * (10 * Hp + 32));
  // a K = 1 handle's one line (kp1_mlp_hparams_store), behind everything else: the allocations above keep the order they always had
  if (K == 1) MLP_ALLOC(m->hparams_dev, HP_FIELDS);
#undef MLP_ALLOC
  if (rc != KP1_OK) {
    kp1_mlp_destroy(m);
    return rc;
  }
  *out = m;
  return KP1_OK;
}
}  // namespace

extern "C" {

int kp1_mlp_destroy(kp1_mlp* m) {
  if (!m) return KP1_OK;
  (void)hipSetDevice(m->device);
  (void)hipDeviceSynchronize();
  for (void* p : m->allocs) (void)hipFree(p);
  for (void* p : {(void*)m->sp_h1, (void*)m->sp_dz2, (void*)m->sp_dz1, (void*)m->sp_xf}) (void)hipFree(p);
  for (auto& v : m->prof)
    for (auto& pr : v) {
      (void)hipEventDestroy(pr.a);
      (void)hipEventDestroy(pr.b);
    }
  delete m;
  return KP1_OK;
}

int kp1_mlp_set_option(kp1_mlp* m, int32_t option, int32_t value) {
  if (!m) return fail(KP1_ERR_INVALID, "NULL argument");
  if (option == KP1_MLP_OPT_FUSED) {
    m->fused = value ? 1 : 0;
    if (!m->fused && m->slab_stale && m->last_params) {   // the layer-wise kernels read the k-slab copies: bring them up to date
      HIP_TRY(hipSetDevice(m->device));
      HIP_TRY(hipDeviceSynchronize());
      Packed k = m->k;
      k.formats = PACK_SLAB | PACK_FRAG;
      hipLaunchKernelGGL(pack_kernel<false>, dim3((unsigned)((m->L.total + 255) / 256)), dim3(256), 0, (hipStream_t)0, m->last_params, m->L, k);
      HIP_TRY(kp1::launch_status());
      HIP_TRY(hipDeviceSynchronize());
      m->slab_stale = false;
    }
    return KP1_OK;
  }
  if (option == KP1_MLP_OPT_BF16X3_WGRAD) {
    if (value && m->K > 1) return fail(KP1_ERR_UNSUPPORTED, "the bf16x3 weight-gradient experiment is not available on population handles");
    if (value && !(m->fused && m->Hp == FU_HP)) return fail(KP1_ERR_UNSUPPORTED, "the bf16x3 weight-gradient experiment needs the 2x256 tile kernels");
    if (value && m->hparams_on) return fail(KP1_ERR_UNSUPPORTED, "the bf16x3 weight-gradient experiment has no hyper-parameter line form (kp1_mlp_hparams_store)");
    if (value && !m->sp_h1) {
      HIP_TRY(hipSetDevice(m->device));
      const size_t act = (size_t)3 * 2 * m->max_batch * m->Hp * sizeof(unsigned short), xb = (size_t)3 * m->max_batch * m->L.INP * sizeof(unsigned short);
      for (unsigned short** p : {&m->sp_h1, &m->sp_dz2, &m->sp_dz1}) {
        HIP_TRY(hipMalloc((void**)p, act));
        HIP_TRY(hipMemset(*p, 0, act));
      }
      HIP_TRY(hipMalloc((void**)&m->sp_xf, xb));
      HIP_TRY(hipMemset(m->sp_xf, 0, xb));
    }
    m->bf16x3 = value ? 1 : 0;
    return KP1_OK;
  }
  if (option == KP1_MLP_OPT_TRAIN_TILE) {
    if (m->Hp != ES_HP) return fail(KP1_ERR_UNSUPPORTED, "KP1_MLP_OPT_TRAIN_TILE is for hidden 64 / 128 handles: hidden 256 has its own tile path (KP1_MLP_OPT_FUSED)");
    m->train_tile = value ? 1 : 0;
    return KP1_OK;
  }
  if (option == KP1_MLP_OPT_PROFILE) {
    m->profile = value ? 1 : 0;
    for (int k = 0; k < KP1_MLP_PROFILE_SLOTS; ++k) m->prof_used[k] = 0;
    return KP1_OK;
  }
  if (option == KP1_MLP_OPT_STEP_COUNT) {   // optimiser steps taken so far (resuming from a checkpoint's Adam state)
    if (value < 0) return fail(KP1_ERR_INVALID, "step count must be >= 0");
    HIP_TRY(hipSetDevice(m->device));
    // a gated handle counts per replica: every line (line 0 is the one every ungated kernel reads)
    for (int r = 0; r < (m->gate_on ? m->K : 1); ++r) HIP_TRY(hipMemcpy(m->step_dev + r * STEP_DEV_INTS, &value, sizeof(int), hipMemcpyHostToDevice));
    return KP1_OK;
  }
  if (option == KP1_MLP_OPT_ACTOR_EXTRA_STEPS) {
    if (value < 0) return fail(KP1_ERR_INVALID, "actor extra steps must be >= 0");
    if (value && m->gate_on) return fail(KP1_ERR_UNSUPPORTED, "actor extra steps are not covered while a KL gate is set on the handle");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpy(m->step_dev + 1, &value, sizeof(int), hipMemcpyHostToDevice));
    m->actor_extra_host = value;
    return KP1_OK;
  }
  return fail(KP1_ERR_INVALID, "unknown kp1_mlp option");
}

int kp1_mlp_set_replica_hparams(kp1_mlp* m, const kp1_replica_hparams* host, int32_t n, void* stream) {
  static_assert(sizeof(kp1_replica_hparams) == sizeof(float) * HP_FIELDS, "kp1_replica_hparams is HP_FIELDS floats");
  static_assert(offsetof(kp1_replica_hparams, learning_rate) == sizeof(float) * HP_LR && offsetof(kp1_replica_hparams, adam_eps) == sizeof(float) * HP_EPS &&
                offsetof(kp1_replica_hparams, max_grad_norm) == sizeof(float) * HP_MAX_NORM && offsetof(kp1_replica_hparams, clip_range) == sizeof(float) * HP_CLIP &&
                offsetof(kp1_replica_hparams, ent_coef) == sizeof(float) * HP_ENT && offsetof(kp1_replica_hparams, vf_coef) == sizeof(float) * HP_VF,
                "kp1_replica_hparams field order");
  if (!m) return fail(KP1_ERR_INVALID, "NULL argument");
  if (n == 0) {   // back to the scalar arguments of kp1_mlp_loss_grad / kp1_mlp_adam_step
    m->hparams_on = false;
    return KP1_OK;
  }
  if (m->K == 1) return fail(KP1_ERR_UNSUPPORTED, "a K = 1 handle takes its hyper-parameters as scalar arguments, not a per-replica table");
  if (n != m->K || !host) return fail(KP1_ERR_INVALID, "kp1_mlp_set_replica_hparams needs one entry per replica (n = K)");
  for (int r = 0; r < n; ++r) {
    const kp1_replica_hparams& h = host[r];
    for (float v : {h.learning_rate, h.adam_eps, h.max_grad_norm, h.clip_range, h.ent_coef, h.vf_coef})
      if (!std::isfinite(v)) return fail(KP1_ERR_INVALID, "replica hyper-parameters must be finite");
  }
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  // stream order: launches already queued on `stream` read the previous table; the copy is complete (host buffer released) on return
  HIP_TRY(hipMemcpyAsync(m->hparams_dev, host, sizeof(kp1_replica_hparams) * (size_t)n, hipMemcpyHostToDevice, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  m->hparams_on = true;
  return KP1_OK;
}

int kp1_mlp_pack_weights(kp1_mlp* m, const float* params, void* stream) {
  if (!m || !params) return fail(KP1_ERR_INVALID, "NULL argument");
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  Packed k = m->k;
  k.formats = PACK_SLAB | PACK_FRAG;
  if (m->K > 1)
    hipLaunchKernelGGL(pack_kernel<true>, dim3((unsigned)((m->L.total + 255) / 256), m->K), dim3(256), 0, (hipStream_t)stream, params, m->L, k);
  else
    hipLaunchKernelGGL(pack_kernel<false>, dim3((unsigned)((m->L.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, params, m->L, k);
  HIP_TRY(kp1::launch_status());
  m->last_params = params;
  m->slab_stale = false;
  return KP1_OK;
}

int kp1_mlp_forward(kp1_mlp* m, const float* obs, int32_t obs_stride, int32_t n, const float* noise, float* mean, float* value, float* action,
                    float* clipped_action, float* log_prob, void* stream) {
  if (!m || !obs) return fail(KP1_ERR_INVALID, "NULL argument");
  int rc = check_batch_args(m, n, obs_stride);
  if (rc != KP1_OK) return rc;
  rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  if (m->fused && m->Hp == FU_HP) {
    FusedArgs fa{};
    fill_fused_head(fa, m, obs, obs_stride, nullptr, n);
    fa.noise = noise; fa.mean = mean; fa.value = value; fa.action = action; fa.clipped = clipped_action; fa.log_prob = log_prob;
    rc = launch_fused_infer(fa, (hipStream_t)stream);
    if (rc != KP1_OK) return rc;
    HIP_TRY(kp1::launch_status());
    return KP1_OK;
  }
  rc = launch_forward_layers(m, obs, obs_stride, nullptr, n, (hipStream_t)stream);
  if (rc != KP1_OK) return rc;
  HeadArgs a{};
  a.h2 = m->h2; a.strideH = (int64_t)m->max_batch * m->Hp; a.Hp = m->Hp; a.n = n; a.H = m->H;
  a.w3 = m->k.w3; a.b3 = m->k.b3; a.log_std = m->k.log_std;
  a.noise = noise; a.mean = mean; a.value = value; a.action = action; a.clipped = clipped_action; a.log_prob = log_prob;
  const bool pop = m->K > 1;
  if (pop) a.r_act = (unsigned)(2 * a.strideH);
  hipLaunchKernelGGL(pop ? head_infer_kernel<true> : head_infer_kernel<false>, dim3((n + HEAD_ROWS - 1) / HEAD_ROWS, m->K), dim3(256),
                     sizeof(float) * HEADS * m->Hp, (hipStream_t)stream, a);
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}

}  // extern "C"

namespace {
// kp1_mlp_forward_env_step on an Hp = 128 handle (hidden 64 / 128, K = 1 or a population): rollout_step_kernel
int forward_env_step_layers(kp1_mlp* m, kp1_env* env, const float* obs, int32_t obs_stride, const float* noise, float* value, float* action,
                            float* log_prob, float* next_obs, float* reward, uint8_t* done, float* terminal_obs, hipStream_t stream) {
  if (m->L.INP != ES_INP)
    return fail(KP1_ERR_UNSUPPORTED, "kp1_mlp_forward_env_step needs the 56-float observation (padded to 64); the 80-float route observation takes the launch sequence");
  if (!noise) return fail(KP1_ERR_INVALID, "NULL argument to kp1_mlp_forward_env_step (the layer-wise form samples: noise is required)");
  if (obs_stride != m->L.IN && obs_stride != m->L.INP) return fail(KP1_ERR_INVALID, "obs_stride must be 56 or 64");
  if (next_obs == obs) return fail(KP1_ERR_INVALID, "kp1_mlp_forward_env_step: the layer-wise form reads obs from two workgroups per tile, next_obs must not be obs");
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  RolloutStepArgs a{};
  int mode = 0, device = 0, pop_replicas = 0, pop_form = 0;
  int64_t n_envs = 0;
  // refuses f64 handles, recorded reward components and a bound handle in a mode kp1_step refuses
  rc = kp1::env_step_args_f32_population(env, &a.env, sizeof a.env, next_obs, reward, done, terminal_obs, 1, &mode, &n_envs, &device, &pop_replicas, &pop_form);
  if (rc != KP1_OK) return rc;
  if (device != m->device) return fail(KP1_ERR_INVALID, "the env handle and the MLP workspace live on different devices");
  if (mode != KP1_MODE_APPROACH && mode != KP1_MODE_DOCK) return fail(KP1_ERR_UNSUPPORTED, "kp1_mlp_forward_env_step steps the approach or the dock mode");
  if (pop_replicas > 0 && pop_replicas != m->K)
    return fail(KP1_ERR_INVALID, "kp1_mlp_forward_env_step: the env handle's population replica count differs from the MLP handle's");
  if (n_envs <= 0 || n_envs % m->K != 0) return fail(KP1_ERR_INVALID, "kp1_mlp_forward_env_step: the env count must be a multiple of the handle's replica count");
  if (n_envs / m->K > m->max_batch) return fail(KP1_ERR_INVALID, "more envs than the workspace max_batch");
  {  // the value net's workgroups read obs rows while the policy net's write next_obs / terminal_obs rows of other tiles: no overlap at all
    const float* obs_end = obs + n_envs * obs_stride;
    const int64_t out_floats = n_envs * a.env.obs_stride;
    auto overlaps = [&](const float* p) { return p && p < obs_end && obs < p + out_floats; };
    if (overlaps(next_obs) || overlaps(terminal_obs))
      return fail(KP1_ERR_INVALID, "kp1_mlp_forward_env_step: next_obs and terminal_obs must not overlap obs in the layer-wise form");
  }
  fill_rollout_forward(a, m, obs, obs_stride, noise, value, action, log_prob, (int)(n_envs / m->K));
  const dim3 grid((unsigned)((a.n + ES_BM - 1) / ES_BM), (unsigned)m->K, value ? 2u : 1u);
  const bool dock = mode == KP1_MODE_DOCK;
  auto* kernel = pop_form != 0 ? (dock ? rollout_step_kernel<KP1_MODE_DOCK, true> : rollout_step_kernel<KP1_MODE_APPROACH, true>)
                               : (dock ? rollout_step_kernel<KP1_MODE_DOCK, false> : rollout_step_kernel<KP1_MODE_APPROACH, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(ES_NTH), 0, stream, a);
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}
}  // namespace

namespace {
template <int INP>
void launch_route_rollout_step(bool pop, dim3 grid, hipStream_t stream, const RouteRolloutStepArgs& a) {
  if (pop) hipLaunchKernelGGL((route_rollout_step_kernel<INP, true>), grid, dim3(ES_NTH), 0, stream, a);
  else hipLaunchKernelGGL((route_rollout_step_kernel<INP, false>), grid, dim3(ES_NTH), 0, stream, a);
}

// ---- what the route one-launch forms share (kp1_mlp_forward_route_step; kp1_mlp_forward_route_chain_step / kp1_route_chain_run), in two phases
// that each caller interleaves with its own refusals.  `who` names the entry point in the refusal texts; they are only built on a refusal.

std::string refusal_text(const char* head, const char* tail) { return std::string(head) + tail; }

// phase 1: the observation layout of the policy handle against the route handle's; *obs_dim = the route observation's width
int route_fwd_check_obs(const char* who, const kp1_mlp* m, const kp1_route* r, int obs_stride, int* obs_dim) {
  *obs_dim = r->cfg.include_route_keys ? KP1_ROUTE_OBS_DIM : KP1_OBS_DIM;
  if (m->L.IN != *obs_dim) return fail(KP1_ERR_INVALID, refusal_text(who, ": the MLP handle's obs_dim differs from the route handle's"));
  if (obs_stride != m->L.IN && obs_stride != m->L.INP)
    return fail(KP1_ERR_INVALID, refusal_text(who, ": obs_stride must be the observation width (56 / 80) or its padded width (64 / 128)"));
  if (obs_stride != r->obs_stride) return fail(KP1_ERR_INVALID, refusal_text(who, ": obs_stride differs from the route handle's (kp1_route_set_obs_stride)"));
  return KP1_OK;
}

// phase 2, after the caller's last refusal that needs no device: the device, the base env's argument block and the refusals that read it, then the
// forward fields of f and the route step's block s.  Nothing is launched.  The caller still applies its overlap rule (over r->n rows) and
// dispatches on the padded width; *pop_form != 0: the base env steps in its population form.
int route_fwd_prepare(const char* who, kp1_mlp* m, kp1_route* r, int obs_dim, const float* obs, int obs_stride, const float* noise, float* value,
                      float* action, float* log_prob, float* next_obs, float* reward, uint8_t* done, float* terminal_obs, int auto_reset,
                      RolloutStepArgs& f, RouteStepArgs<float>& s, int* pop_form) {
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  int mode = 0, device = 0, pop_replicas = 0;
  int64_t n_envs = 0;
  // the base step as route_launch_step launches it: the wrapper's scratch at pitch 56, no terminal observation, no auto-reset.  Refuses f64
  // base handles, recorded base reward components and a bound handle in a mode kp1_step refuses.
  rc = kp1::env_step_args_f32_population(r->base, &f.env, sizeof f.env, r->base_obs, r->base_reward, r->bytes + 4 * r->n, nullptr, 0, &mode, &n_envs,
                                         &device, &pop_replicas, pop_form);
  if (rc != KP1_OK) return rc;
  f.env.obs_stride = KP1_OBS_DIM;
  if (device != m->device) return fail(KP1_ERR_INVALID, "the route handle and the MLP workspace live on different devices");
  if (mode != KP1_MODE_APPROACH) return fail(KP1_ERR_UNSUPPORTED, refusal_text(who, ": the route wrappers drive an approach-mode base env"));
  if (pop_replicas > 0 && pop_replicas != m->K)
    return fail(KP1_ERR_INVALID, refusal_text(who, ": the base env's population replica count differs from the MLP handle's"));
  if (n_envs != r->n || n_envs <= 0 || n_envs % m->K != 0)
    return fail(KP1_ERR_INVALID, refusal_text(who, ": the env count must be a multiple of the handle's replica count"));
  if (n_envs / m->K > m->max_batch) return fail(KP1_ERR_INVALID, "more envs than the workspace max_batch");
  if (!r->fused_actions) return fail(KP1_ERR_UNSUPPORTED, refusal_text(who, " runs on an fp32 route handle"));
  fill_rollout_forward(f, m, obs, obs_stride, noise, value, action, log_prob, (int)(n_envs / m->K));
  s.st = f.env.st; s.cfg = f.env.cfg; s.smp = f.env.smp; s.rc = r->dev_cfg; s.rt = route_table_of(r); s.rs = route_state_of<float>(r);
  s.actions = r->fused_actions; s.base_done = r->bytes + 4 * r->n; s.obs = next_obs; s.reward = reward; s.done = done; s.terminal_obs = terminal_obs;
  s.obs_dim = obs_dim; s.obs_stride = r->obs_stride; s.auto_reset = auto_reset;
  return KP1_OK;
}
}  // namespace

extern "C" {

// kp1_mlp_forward + kp1_route_step(auto_reset = 1) in one launch (include/kp1_route.h): route_rollout_step_kernel
int kp1_mlp_forward_route_step(kp1_mlp* m, kp1_route* r, const float* obs, int32_t obs_stride, const float* noise, float* value, float* action,
                               float* log_prob, float* next_obs, float* reward, uint8_t* done, float* terminal_obs, void* stream) {
  if (!m || !r || !obs || !noise || !action || !next_obs || !reward || !done) return fail(KP1_ERR_INVALID, "NULL argument to kp1_mlp_forward_route_step");
  if (m->Hp != ES_HP) return fail(KP1_ERR_UNSUPPORTED, "kp1_mlp_forward_route_step covers hidden 64 / 128 (the layer-wise layout); hidden 256 takes the launch sequence");
  const char* who = "kp1_mlp_forward_route_step";
  int obs_dim = 0;
  int rc = route_fwd_check_obs(who, m, r, obs_stride, &obs_dim);
  if (rc != KP1_OK) return rc;
  if (r->comps_enabled) return fail(KP1_ERR_UNSUPPORTED, "kp1_mlp_forward_route_step does not record route reward components (kp1_route_enable_reward_components is on)");
  if (r->n_chains > 0) return fail(KP1_ERR_UNSUPPORTED, "kp1_mlp_forward_route_step: the route handle has a live kp1_route_chain");
  if (r->n_waypoints > KP1_ROUTE_FUSED_MAX_WAYPOINTS)
    return fail(KP1_ERR_UNSUPPORTED, "kp1_mlp_forward_route_step: the route has more than KP1_ROUTE_FUSED_MAX_WAYPOINTS waypoints (the joint table overlays the kernel's LDS tiles)");
  if (r->n_replicas != m->K) return fail(KP1_ERR_INVALID, "kp1_mlp_forward_route_step: the route handle's replica count differs from the MLP handle's");
  if (next_obs == obs) return fail(KP1_ERR_INVALID, "kp1_mlp_forward_route_step reads obs from two workgroups per tile, next_obs must not be obs");
  RouteRolloutStepArgs a{};
  RolloutStepArgs& f = a.fwd;
  int pop_form = 0;
  rc = route_fwd_prepare(who, m, r, obs_dim, obs, obs_stride, noise, value, action, log_prob, next_obs, reward, done, terminal_obs, 1, f, a.route, &pop_form);
  if (rc != KP1_OK) return rc;
  {  // the value net's workgroups read obs rows while the policy net's write next_obs / terminal_obs rows of other tiles: no overlap at all
    const float* obs_end = obs + r->n * obs_stride;
    const int64_t out_floats = r->n * r->obs_stride;
    auto overlaps = [&](const float* p) { return p && p < obs_end && obs < p + out_floats; };
    if (overlaps(next_obs) || overlaps(terminal_obs))
      return fail(KP1_ERR_INVALID, "kp1_mlp_forward_route_step: next_obs and terminal_obs must not overlap obs");
  }
  const int INP = m->L.INP;
  a.clipped = r->fused_actions;
  const dim3 grid((unsigned)((f.n + ES_BM - 1) / ES_BM), (unsigned)m->K, value ? 2u : 1u);
  if (INP == ES_INP) launch_route_rollout_step<ES_INP>(pop_form != 0, grid, (hipStream_t)stream, a);
  else if (INP == RR_MAX_INP) launch_route_rollout_step<RR_MAX_INP>(pop_form != 0, grid, (hipStream_t)stream, a);
  else return fail(KP1_ERR_UNSUPPORTED, "kp1_mlp_forward_route_step: unexpected padded observation width");
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}

}  // extern "C"

namespace {
template <int INP, bool EPISODE>
void launch_route_chain_step(bool pop, dim3 grid, hipStream_t stream, const RouteChainStepArgs& a) {
  if (pop) hipLaunchKernelGGL((route_chain_step_kernel<INP, true, EPISODE>), grid, dim3(ES_NTH), 0, stream, a);
  else hipLaunchKernelGGL((route_chain_step_kernel<INP, false, EPISODE>), grid, dim3(ES_NTH), 0, stream, a);
}

// kp1_mlp_forward_route_chain_step (EPISODE false, one lock step) and kp1_route_chain_run (EPISODE true, n_steps of them in place): every refusal,
// then the counter's memset and the one launch
template <bool EPISODE>
int route_chain_step_launch(const char* who, kp1_mlp* m, kp1_route* r, kp1_route_chain* c, const float* obs, int32_t obs_stride, float* action,
                            float* next_obs, float* reward, uint8_t* done, int32_t* tags, int32_t n_steps, hipStream_t stream) {
  if (!m || !r || !c || !obs || !next_obs || !reward || !done) return fail(KP1_ERR_INVALID, refusal_text("NULL argument to ", who));
  if (m->Hp != ES_HP) return fail(KP1_ERR_UNSUPPORTED, refusal_text(who, " covers hidden 64 / 128 (the layer-wise layout); hidden 256 takes the launch sequence"));
  if (const char* why = kp1::route_chain_refusal(r)) return fail(KP1_ERR_UNSUPPORTED, why);
  if (c->owner != r) return fail(KP1_ERR_INVALID, refusal_text(who, ": the chain belongs to another route handle"));
  if ((int64_t)c->n_rows != r->n) return fail(KP1_ERR_INVALID, refusal_text(who, ": the chain was created for another env count"));
  int obs_dim = 0;
  int rc = route_fwd_check_obs(who, m, r, obs_stride, &obs_dim);
  if (rc != KP1_OK) return rc;
  if (r->n_waypoints > KP1_ROUTE_FUSED_MAX_WAYPOINTS)
    return fail(KP1_ERR_UNSUPPORTED, refusal_text(who, ": the route has more than KP1_ROUTE_FUSED_MAX_WAYPOINTS waypoints (the joint table overlays the kernel's LDS tiles)"));
  // a chain's rows are replica-major on any handle: a single route handle of K C envs serves a policy handle of K replicas
  if (r->n_replicas != 1 && r->n_replicas != m->K) return fail(KP1_ERR_INVALID, refusal_text(who, ": the route handle's replica count differs from the MLP handle's"));
  if (EPISODE && (n_steps < 1 || n_steps > KP1_ROUTE_CHAIN_RUN_MAX_STEPS))
    return fail(KP1_ERR_INVALID, refusal_text(who, ": n_steps must be in [1, KP1_ROUTE_CHAIN_RUN_MAX_STEPS] (1024); split a longer chain into consecutive calls"));
  RouteChainStepArgs a{};
  RolloutStepArgs& f = a.fwd;
  int pop_form = 0;
  rc = route_fwd_prepare(who, m, r, obs_dim, obs, obs_stride, nullptr, nullptr, action, nullptr, next_obs, reward, done, nullptr, 0, f, a.route, &pop_form);
  if (rc != KP1_OK) return rc;
  if (next_obs != obs) {  // a workgroup reads and writes its own rows only, all reads before the writes: exact aliasing is the evaluator's normal use
    const float* obs_end = obs + r->n * obs_stride;
    if (next_obs < obs_end && obs < next_obs + r->n * (int64_t)r->obs_stride)
      return fail(KP1_ERR_INVALID, refusal_text(who, ": next_obs must be obs itself (in place) or not overlap it"));
  }
  const int INP = m->L.INP;
  a.ch = c->d; a.tags = tags; a.clipped = r->fused_actions; a.n_steps = EPISODE ? n_steps : 1;
  if (INP != ES_INP && INP != RR_MAX_INP) return fail(KP1_ERR_UNSUPPORTED, refusal_text(who, ": unexpected padded observation width"));
  HIP_TRY(hipMemsetAsync(c->d.n_alive, 0, sizeof(int32_t), stream));
  const dim3 grid((unsigned)((f.n + ES_BM - 1) / ES_BM), (unsigned)m->K);
  if (INP == ES_INP) launch_route_chain_step<ES_INP, EPISODE>(pop_form != 0, grid, stream, a);
  else launch_route_chain_step<RR_MAX_INP, EPISODE>(pop_form != 0, grid, stream, a);
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}
}  // namespace

extern "C" {

// kp1_mlp_forward (noise NULL, clipped) + kp1_route_chain_step in one launch (include/kp1_route.h): route_chain_step_kernel<.., false>
int kp1_mlp_forward_route_chain_step(kp1_mlp* m, kp1_route* r, kp1_route_chain* chain, const float* obs, int32_t obs_stride, float* action,
                                     float* next_obs, float* reward, uint8_t* done, int32_t* tags, void* stream) {
  return route_chain_step_launch<false>("kp1_mlp_forward_route_chain_step", m, r, chain, obs, obs_stride, action, next_obs, reward, done, tags, 1,
                                        (hipStream_t)stream);
}

// n_steps lock steps in one launch, in place on obs: route_chain_step_kernel<.., true>
int kp1_route_chain_run(kp1_mlp* m, kp1_route* r, kp1_route_chain* chain, float* obs, int32_t obs_stride, float* reward, uint8_t* done,
                        int32_t n_steps, void* stream) {
  return route_chain_step_launch<true>("kp1_route_chain_run", m, r, chain, obs, obs_stride, nullptr, obs, reward, done, nullptr, n_steps,
                                       (hipStream_t)stream);
}

}  // extern "C"

extern "C" {

int kp1_mlp_forward_env_step(kp1_mlp* m, kp1_env* env, const float* obs, int32_t obs_stride, const float* noise, float* value, float* action,
                             float* log_prob, float* next_obs, float* reward, uint8_t* done, float* terminal_obs, void* stream) {
  if (!m || !env || !obs || !action || !next_obs || !reward || !done) return fail(KP1_ERR_INVALID, "NULL argument to kp1_mlp_forward_env_step");
  // hidden 64 / 128 (K = 1 or a population): the layer-wise form; every population handle has this layout
  if (m->Hp == ES_HP) return forward_env_step_layers(m, env, obs, obs_stride, noise, value, action, log_prob, next_obs, reward, done, terminal_obs, (hipStream_t)stream);
  if (!(m->fused && m->Hp == FU_HP) || m->L.INP != 64)
    return fail(KP1_ERR_UNSUPPORTED, "kp1_mlp_forward_env_step needs the 2x256 tile kernels and the 56-float observation (padded to 64)");
  if (obs_stride != m->L.IN && obs_stride != m->L.INP) return fail(KP1_ERR_INVALID, "obs_stride must be 56 or 64");
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  FusedArgs fa{};
  int mode = 0, device = 0;
  int64_t n_envs = 0;
  rc = kp1::env_step_args_f32(env, &fa.env, sizeof fa.env, nullptr, next_obs, reward, done, terminal_obs, 1, &mode, &n_envs, &device);
  if (rc != KP1_OK) return rc;
  if (device != m->device) return fail(KP1_ERR_INVALID, "the env handle and the MLP workspace live on different devices");
  if (n_envs > m->max_batch) return fail(KP1_ERR_INVALID, "more envs than the workspace max_batch");
  fill_fused_head(fa, m, obs, obs_stride, nullptr, (int)n_envs);
  fa.noise = noise; fa.value = value; fa.action = action; fa.log_prob = log_prob;
  rc = launch_fused_infer_env(fa, mode, (hipStream_t)stream);
  if (rc != KP1_OK) return rc;
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}

// all env steps of a rollout span in one launch, the critic of the span in a second: rollout_run_kernel +
// rollout_value_kernel.  Every refusal comes before the first launch.
int kp1_rollout_run(kp1_mlp* m, kp1_env* env, float* obs, int32_t obs_stride, const float* noise, float* value, float* action, float* log_prob,
                    float* reward, uint8_t* done, float* terminal_obs, int32_t n_steps, kp1_curriculum_state* trackers, int32_t steps_per_call,
                    void* stream) {
  if (!m || !env || !obs || !noise || !action || !reward || !done) return fail(KP1_ERR_INVALID, "NULL argument to kp1_rollout_run");
  if (n_steps < 1 || n_steps > KP1_ROLLOUT_RUN_MAX_STEPS)
    return fail(KP1_ERR_INVALID, "kp1_rollout_run: one call runs 1 to KP1_ROLLOUT_RUN_MAX_STEPS (2048) env steps; split a longer rollout into consecutive calls");
  if (m->Hp != ES_HP) return fail(KP1_ERR_UNSUPPORTED, "kp1_rollout_run covers hidden 64 / 128; hidden 256 takes kp1_mlp_forward_env_step per step");
  if (m->L.INP != ES_INP) return fail(KP1_ERR_UNSUPPORTED, "kp1_rollout_run needs the 56-float observation (padded to 64), not the 80-float route observation");
  if (obs_stride != m->L.IN && obs_stride != m->L.INP) return fail(KP1_ERR_INVALID, "kp1_rollout_run: obs_stride must be 56 or 64");
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  RolloutRunArgs a{};
  int mode = 0, device = 0, pop_replicas = 0, pop_form = 0;
  int64_t n_envs = 0;
  // refuses f64 handles, recorded reward components and a bound handle in a mode kp1_step refuses
  rc = kp1::env_step_args_f32_population(env, &a.s.env, sizeof a.s.env, nullptr, reward, done, terminal_obs, 1, &mode, &n_envs, &device, &pop_replicas, &pop_form);
  if (rc != KP1_OK) return rc;
  if (device != m->device) return fail(KP1_ERR_INVALID, "the env handle and the MLP workspace live on different devices");
  if (mode != KP1_MODE_APPROACH || a.s.env.pop_dock)
    return fail(KP1_ERR_UNSUPPORTED, "kp1_rollout_run steps the approach mode; the dock mode and handles bound to dock stage records take kp1_mlp_forward_env_step per step");
  if (pop_replicas > 0 && pop_replicas != m->K)
    return fail(KP1_ERR_INVALID, "kp1_rollout_run: the env handle's population replica count differs from the MLP handle's");
  if (n_envs <= 0 || n_envs % m->K != 0) return fail(KP1_ERR_INVALID, "kp1_rollout_run: the env count must be a multiple of the handle's replica count");
  const int64_t n = n_envs / m->K;
  if (n > m->max_batch) return fail(KP1_ERR_INVALID, "more envs than the workspace max_batch");
  if (a.s.env.obs_stride != obs_stride)
    return fail(KP1_ERR_INVALID, "kp1_rollout_run: obs_stride must be the env handle's observation pitch (step t + 1 reads what step t's env step wrote)");
  if (terminal_obs) {
    const float* obs_end = obs + (int64_t)(n_steps + 1) * n_envs * obs_stride;
    if (terminal_obs < obs_end && obs < terminal_obs + (int64_t)n_steps * n_envs * obs_stride)
      return fail(KP1_ERR_INVALID, "kp1_rollout_run: terminal_obs must not overlap the obs buffer");
  }
  if (trackers) {
    if (n > ES_BM)
      return fail(KP1_ERR_UNSUPPORTED, "kp1_rollout_run folds the tracker in only when a replica is one tile (at most 32 envs per replica); observe per step above that");
    const void *bound_stage = nullptr, *bound_pop = nullptr;
    kp1::env_bound_stage_source(env, &bound_stage, &bound_pop);
    const bool ours = m->K == 1 ? (bound_stage == (const void*)&trackers->stage_index || bound_pop == (const void*)trackers) : bound_pop == (const void*)trackers;
    if (!ours)
      return fail(KP1_ERR_INVALID, "kp1_rollout_run: the env handle's bound stage source is not `trackers` (&trackers->stage_index for K = 1, the K states for a population)");
    if (steps_per_call < 0) return fail(KP1_ERR_INVALID, "kp1_rollout_run: steps_per_call is negative");
  }
  fill_rollout_forward(a.s, m, obs, obs_stride, noise, value, action, log_prob, (int)n);
  a.s.env.obs = obs + n_envs * obs_stride;          // slice 1: step 0's next_obs
  a.rows = n_envs;
  a.n_steps = n_steps;
  a.steps_per_call = steps_per_call;
  a.trackers = trackers;
  a.track_stage = (a.s.env.stage_ptr != nullptr || pop_form != 0) ? 1 : 0;
  const dim3 grid((unsigned)((a.s.n + ES_BM - 1) / ES_BM), (unsigned)m->K);
  auto* kernel = trackers ? rollout_run_kernel<false, true> : (pop_form != 0 ? rollout_run_kernel<true, false> : rollout_run_kernel<false, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(ES_NTH), 0, (hipStream_t)stream, a);
  if (value) hipLaunchKernelGGL(rollout_value_kernel, dim3(grid.x, grid.y, (unsigned)n_steps), dim3(ES_NTH), 0, (hipStream_t)stream, a);
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}

}  // extern "C"

namespace {
// what kp1_eval_step and kp1_eval_episodes share: every refusal, and the launch arguments of the handle's form
struct EvalLaunch {
  bool tile;                // hidden 256: the evaluation forms of the tile kernel; hidden 64 / 128: eval_step_kernel
  int mode, K;
  EvalStepArgs a;
  FusedArgs fa;
};

// refuses what neither entry point can run (nothing has been launched); on KP1_OK *L holds the arguments of env steps step .. last_step.
// The step range is checked where kp1_eval_step has always checked its step: after the NULL checks, before a handle is looked at
int eval_prepare(kp1_mlp* m, kp1_env* env, float* obs, float* reward, uint8_t* done, const kp1_eval_buffers* b, int32_t step, int32_t last_step,
                 bool episodes, const double* ready_thresholds, int32_t confirm_steps, EvalLaunch* L) {
  if (!m || !env || !obs || !reward || !done || !b) return fail(KP1_ERR_INVALID, "NULL argument to kp1_eval_step");
  if (!b->metrics || !b->counters || !b->flags || !b->state || !b->n_alive) return fail(KP1_ERR_INVALID, "kp1_eval_step: NULL buffer");
  if (b->hand_metrics && (!b->hand_step || !b->hand_success || !b->hand_state)) return fail(KP1_ERR_INVALID, "kp1_eval_step: incomplete handoff buffers");
  if (!episodes) {
    if (step < 1) return fail(KP1_ERR_INVALID, "kp1_eval_step accounts env steps 1, 2, ...: step 0 (the initialisation after a reset) is kp1_eval_accumulate's");
  } else {
    if (step < 1) return fail(KP1_ERR_INVALID, "kp1_eval_episodes: first_step must be at least 1 (step 0, the initialisation after a reset, is kp1_eval_accumulate's)");
    if (last_step < step) return fail(KP1_ERR_INVALID, "kp1_eval_episodes: last_step is below first_step");
    if ((int64_t)last_step - step + 1 > KP1_EVAL_EPISODES_MAX_STEPS)
      return fail(KP1_ERR_INVALID, "kp1_eval_episodes: one call runs at most KP1_EVAL_EPISODES_MAX_STEPS (256) env steps; split a longer span into consecutive calls");
  }
  const bool tile = m->Hp == FU_HP;
  if (!tile && m->Hp != ES_HP) return fail(KP1_ERR_UNSUPPORTED, "kp1_eval_step covers hidden 64 / 128 (layer-wise layout) and 256 (tile kernels)");
  if (tile && (m->K > 1 || !m->fused))
    return fail(KP1_ERR_UNSUPPORTED, "kp1_eval_step: the 256 form needs the tile kernels (a K = 1 handle with the tile path on); this handle runs the layer-wise kernels");
  if (m->L.INP != ES_INP) return fail(KP1_ERR_UNSUPPORTED, "kp1_eval_step needs the 56-float observation (padded to 64)");
  EvalStepArgs& a = L->a;
  a = EvalStepArgs{};
  int mode = 0, device = 0;
  int64_t n_envs = 0;
  // refuses f64 handles, recorded reward components and env handles with bound population stages
  int rc = kp1::env_step_args_f32(env, &a.env, sizeof a.env, nullptr, obs, reward, done, nullptr, 0, &mode, &n_envs, &device);
  if (rc != KP1_OK) return rc;
  if (a.env.stage_ptr) return fail(KP1_ERR_UNSUPPORTED, "kp1_eval_step: the env handle is bound to a curriculum tracker (an evaluation handle has none)");
  if (device != m->device) return fail(KP1_ERR_INVALID, "the env handle and the MLP workspace live on different devices");
  if (mode != KP1_MODE_APPROACH && mode != KP1_MODE_DOCK) return fail(KP1_ERR_UNSUPPORTED, "kp1_eval_step steps the approach or the dock mode");
  if (n_envs <= 0 || n_envs % m->K != 0) return fail(KP1_ERR_INVALID, "kp1_eval_step: the env count must be a multiple of the handle's replica count");
  rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  L->tile = tile; L->mode = mode; L->K = m->K;
  if (tile) {
    FusedArgs& fa = L->fa;
    fa = FusedArgs{};
    fa.env = a.env;
    fill_fused_head(fa, m, obs, a.env.obs_stride, nullptr, (int)n_envs);
    fa.ev.b = *b;
    fa.ev.step = step; fa.ev.last_step = last_step; fa.ev.confirm = confirm_steps;
    fa.ev.track_ready = ready_thresholds != nullptr;
    if (ready_thresholds) { fa.ev.thr_pos = ready_thresholds[0]; fa.ev.thr_ori = ready_thresholds[1]; fa.ev.thr_act = ready_thresholds[2]; fa.ev.thr_dq = ready_thresholds[3]; }
    return KP1_OK;
  }
  a.b = *b;
  fill_layer_weights(a, m);
  a.n = (int)(n_envs / m->K);
  a.Kreal = kreal(m, a.env.obs_stride);
  a.step = step; a.last_step = last_step; a.confirm = confirm_steps;
  a.track_ready = ready_thresholds != nullptr;
  if (ready_thresholds) { a.thr_pos = ready_thresholds[0]; a.thr_ori = ready_thresholds[1]; a.thr_act = ready_thresholds[2]; a.thr_dq = ready_thresholds[3]; }
  return KP1_OK;
}

// zeroes n_alive, then the one launch of the prepared form: the step kernels, or (EPISODE) the whole-episode ones
template <bool EPISODE>
int eval_launch(const EvalLaunch& L, hipStream_t st) {
  if (L.tile) {
    HIP_TRY(hipMemsetAsync(L.fa.ev.b.n_alive, 0, sizeof(int32_t), st));
    // obs is read (x tile, before the first barrier) and overwritten (after the last) in place
    const int rc = EPISODE ? launch_fused_eval_episodes(L.fa, L.mode, st) : launch_fused_eval_env(L.fa, L.mode, st);
    if (rc != KP1_OK) return rc;
    HIP_TRY(kp1::launch_status());
    return KP1_OK;
  }
  const EvalStepArgs& a = L.a;
  HIP_TRY(hipMemsetAsync(a.b.n_alive, 0, sizeof(int32_t), st));
  const dim3 grid((unsigned)((a.n + ES_BM - 1) / ES_BM), (unsigned)L.K);
  const bool pop = L.K > 1, dock = L.mode == KP1_MODE_DOCK;
  auto* kernel = pop ? (dock ? eval_step_kernel<KP1_MODE_DOCK, true, EPISODE> : eval_step_kernel<KP1_MODE_APPROACH, true, EPISODE>)
                     : (dock ? eval_step_kernel<KP1_MODE_DOCK, false, EPISODE> : eval_step_kernel<KP1_MODE_APPROACH, false, EPISODE>);
  hipLaunchKernelGGL(kernel, grid, dim3(ES_NTH), 0, st, a);
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}
}  // namespace

extern "C" {

int kp1_eval_step(kp1_mlp* m, kp1_env* env, float* obs, float* reward, uint8_t* done, const kp1_eval_buffers* b, int32_t step,
                  const double* ready_thresholds, int32_t confirm_steps, void* stream) {
  EvalLaunch L;
  const int rc = eval_prepare(m, env, obs, reward, done, b, step, step, false, ready_thresholds, confirm_steps, &L);
  if (rc != KP1_OK) return rc;
  return eval_launch<false>(L, (hipStream_t)stream);
}

int kp1_eval_episodes(kp1_mlp* m, kp1_env* env, float* obs, float* reward, uint8_t* done, const kp1_eval_buffers* b, int32_t first_step,
                      int32_t last_step, const double* ready_thresholds, int32_t confirm_steps, void* stream) {
  EvalLaunch L;
  const int rc = eval_prepare(m, env, obs, reward, done, b, first_step, last_step, true, ready_thresholds, confirm_steps, &L);
  if (rc != KP1_OK) return rc;
  return eval_launch<true>(L, (hipStream_t)stream);
}

int kp1_mlp_loss_grad(kp1_mlp* m, const float* obs, int32_t obs_stride, const int64_t* idx, int32_t n, const float* actions,
                      const float* old_log_prob, const float* advantages, const float* returns, float adv_mean, float adv_inv_std,
                      const float* adv_stats_dev, float clip_range, float ent_coef, float vf_coef, float inv_count, float* grad_out,
                      float* stats_out, int32_t grad_is_zero, void* stream_) {
  if (!m || !obs || !actions || !old_log_prob || !advantages || !returns || !grad_out) return fail(KP1_ERR_INVALID, "NULL argument");
  int rc = check_batch_args(m, n, obs_stride);
  if (rc != KP1_OK) return rc;
  rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int Hp = m->Hp, H = m->H, INP = m->L.INP;
  const int64_t act_stride = (int64_t)m->max_batch * Hp;
  const ParamLayout& L = m->L;
  (void)grad_is_zero;  // every gradient element is written (not accumulated) by grad_finalize_kernel
  const bool fused = m->fused && Hp == FU_HP;
  const bool pop = m->K > 1;
  // a handle whose kernels read the hyper-parameter table: a population with a table, or a K = 1 handle with its line on, which launches
  // the population forms of those kernels with grid.y = 1 (replica 0: every per-replica offset is zero) and the line forms at hidden 256
  const bool table = m->hparams_on, line_on = table && !pop;
  if (pop && !idx) return fail(KP1_ERR_INVALID, "population handles gather their rows through idx [K][n]");
  const int64_t hpart_rep = (int64_t)(m->max_batch / 32) * (10 * Hp + 32);
  int adv_mode = 0;
  if (adv_stats_dev) adv_mode = 2;
  else if (adv_inv_std > 0.f) adv_mode = 3;
  else if (adv_inv_std == 0.f) adv_mode = 1;
  if (adv_mode == 1)
    hipLaunchKernelGGL(pop ? adv_partials_kernel<true> : adv_partials_kernel<false>, dim3(N_PARTIALS, m->K), dim3(256), 0, stream, advantages, idx, n,
                       m->partials, pop ? (unsigned)PARTIALS_STRIDE : 0u);
  const int hpart_stride = 10 * Hp + 32;
  // KP1_MLP_OPT_TRAIN_TILE: chunks of the one-launch tile, or 0 = the layer-wise launches (option off, or more rows than the slabs cover)
  const int tt_chunks = m->train_tile && !fused ? train_tile_chunks(n) : 0;
  if (fused) {
    FusedArgs fa{};
    fill_fused_head(fa, m, obs, obs_stride, idx, n);
    fa.actions = actions; fa.old_logp = old_log_prob; fa.adv = advantages; fa.ret = returns;
    fa.adv_partials = m->partials; fa.n_adv_partials = N_PARTIALS; fa.adv_stats = adv_stats_dev; fa.adv_mean = adv_mean; fa.adv_inv_std = adv_inv_std;
    fa.adv_mode = adv_mode;
    fa.clip_range = clip_range; fa.vf_coef = vf_coef; fa.inv_count = inv_count;
    fa.h1 = m->h1; fa.dz2 = m->dz2; fa.dz1 = m->dz1; fa.act_stride = act_stride; fa.xf = m->xf;
    fa.bslab = m->bslab; fa.hpart = m->hpart; fa.hpart_stride = hpart_stride;
    if (m->bf16x3) {
      fa.sp_h1 = m->sp_h1; fa.sp_dz2 = m->sp_dz2; fa.sp_dz1 = m->sp_dz1; fa.sp_xf = m->sp_xf;
      fa.sp_plane = (int64_t)2 * m->max_batch * Hp; fa.sp_plane_x = (int64_t)m->max_batch * INP;
    }
    {
      ProfScope ps(m, KP1_MLP_PROFILE_TILE, stream);
      rc = line_on ? launch_fused_line(fa, m->hparams_dev, stream) : launch_fused(fa, stream);
    }
    if (rc != KP1_OK) return rc;
  } else {
    HeadArgs a{};
    a.h2 = m->h2; a.strideH = act_stride; a.Hp = Hp; a.n = n; a.H = H;
    a.w3 = m->k.w3; a.b3 = m->k.b3; a.log_std = m->k.log_std;
    a.idx = idx; a.actions = actions; a.old_logp = old_log_prob; a.adv = advantages; a.ret = returns;
    a.adv_partials = m->partials; a.n_adv_partials = N_PARTIALS; a.adv_stats = adv_stats_dev; a.adv_mean = adv_mean; a.adv_inv_std = adv_inv_std;
    a.adv_mode = adv_mode;
    a.clip_range = clip_range; a.ent_coef = ent_coef; a.vf_coef = vf_coef; a.inv_count = inv_count;
    a.dz2 = m->dz2;
    a.hpart = m->hpart; a.hpart_stride = hpart_stride;
    a.r_act = (unsigned)(2 * act_stride); a.r_hpart = (unsigned)hpart_rep; a.r_partials = (unsigned)PARTIALS_STRIDE;
    a.hparams = table ? m->hparams_dev : nullptr;
    if (tt_chunks) {
      ProfScope ps(m, KP1_MLP_PROFILE_TILE, stream);
      rc = launch_train_tile(m, a, obs, obs_stride, tt_chunks, grad_out, stream);
      if (rc != KP1_OK) return rc;
    } else {
      rc = launch_forward_layers(m, obs, obs_stride, idx, n, stream);
      if (rc != KP1_OK) return rc;
      const dim3 hgrid((n + HEAD_ROWS - 1) / HEAD_ROWS, m->K);
      const size_t hbytes = sizeof(float) * (HEADS * Hp + HEAD_ROWS * 8 + 84 + 2 * HEAD_ROWS * (Hp + 4));
      // pop: Hp = 128 (kp1_mlp_create_population)
      auto* kernel = head_train_kernel<128, true>;
      if (!pop && !line_on) kernel = Hp == 256 ? head_train_kernel<256> : head_train_kernel<128>;
      if (line_on && Hp == 256) {
        rc = kp1::mlp_line_launch_head_train256(&a, sizeof(a), hgrid, hbytes, stream);   // head_train_kernel<256, true>: kp1_mlp_line.hip
        if (rc != KP1_OK) return rc;
      } else {
        HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hbytes));
        hipLaunchKernelGGL(kernel, hgrid, dim3(256), hbytes, stream, a);
      }
      rc = launch_nt<EPI_DTANH>(backward_nt_args(m, n), stream);
      if (rc != KP1_OK) return rc;
    }
  }

  // weight gradients (split over the batch axis)
  int s2_n = 0, s1_n = 0;
  if (fused) {
    const TnFragArgs t = tn_frag_args(m, n);
    if (m->bf16x3) {   // [r3 experiment] same slabs, same chunking in 16-row fragments
      TnBf16Args b{};
      b.dz2 = m->sp_dz2; b.h1 = m->sp_h1; b.dz1 = m->sp_dz1; b.plane = (int64_t)2 * m->max_batch * Hp; b.net = (int64_t)m->max_batch * Hp;
      b.xf = m->sp_xf; b.plane_x = (int64_t)m->max_batch * INP; b.inp = INP;
      b.slab2 = t.slab2; b.s2_net = t.s2_net; b.s2_chunk = t.s2_chunk; b.slab1 = t.slab1; b.s1_net = t.s1_net; b.s1_chunk = t.s1_chunk;
      b.frags = t.groups / 2; b.cf2 = t.cg2 / 2; b.cf1 = t.cg1 / 2; b.n_chunks2 = t.n_chunks2; b.n_chunks1 = t.n_chunks1;   // groups, cg2, cg1 are multiples of 4 / 8
      const size_t bytes = sizeof(float) * TN_SPLIT_LDS_FLOATS;
      HIP_TRY(hipFuncSetAttribute((const void*)gemm_tn_bf16x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
      ProfScope ps(m, KP1_MLP_PROFILE_WGRAD, stream);
      KP1_LAUNCH(gemm_tn_bf16x3_kernel, dim3(32 * b.n_chunks2 + 16 * b.n_chunks1), dim3(256), bytes, stream, b);
    } else {
      ProfScope ps(m, KP1_MLP_PROFILE_WGRAD, stream);
      rc = launch_tn_frag(t, stream);
    }
    if (rc != KP1_OK) return rc;
    s2_n = t.n_chunks2;
    s1_n = t.n_chunks1;
  } else if (tt_chunks) {
    s2_n = s1_n = tt_chunks;   // train_tile128_kernel left one slab of each per chunk
  } else {
    rc = launch_layer_wgrads(m, obs, obs_stride, idx, n, &s2_n, &s1_n, stream);
    if (rc != KP1_OK) return rc;
  }
  FinalizeArgs f{};
  fill_finalize(f, m, n, s2_n, s1_n, grad_out);
  if (fused) f.b_n = (n + FU_BM - 1) / FU_BM * (FU_BM / 32);   // the tile kernel's 32-row tiles
  if (tt_chunks) f.b_n = tt_chunks;                            // one b1 partial row per chunk (= f.h_n: a chunk is one 32-row block)
  f.ent_coef = ent_coef; f.inv_count = inv_count;
  f.stats = stats_out; f.sumsq = m->partials + 2 * N_PARTIALS;
  f.step_counter = m->step_dev;
  f.r_sumsq = (unsigned)PARTIALS_STRIDE;
  f.hparams = table ? m->hparams_dev : nullptr;
  const int n_main = (int)((finalize_vec_items(L) + 255) / 256);
  m->n_finalize_blocks = n_main + (int)((finalize_wide_count(L) + 3 + 31) / 32);
  if (m->n_finalize_blocks > 2048) return fail(KP1_ERR_INVALID, "parameter vector too large for the sum-of-squares partial buffer");
  {
    ProfScope ps(m, KP1_MLP_PROFILE_FINALIZE, stream);
    if (m->gate_on) {
      auto* kernel = pop || line_on ? grad_finalize_gated_kernel<true> : grad_finalize_gated_kernel<false>;
      KP1_LAUNCH(kernel, dim3(m->n_finalize_blocks, m->K), dim3(256), 0, stream, f, n_main, m->gate_dev);
    } else {
      auto* kernel = pop || line_on ? grad_finalize_kernel<true> : grad_finalize_kernel<false>;
      KP1_LAUNCH(kernel, dim3(m->n_finalize_blocks, m->K), dim3(256), 0, stream, f, n_main);
    }
  }
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}

int kp1_mlp_profile_read(kp1_mlp* m, float* out_us, int32_t* out_launches) {
  if (!m || !out_us || !out_launches) return fail(KP1_ERR_INVALID, "NULL argument to kp1_mlp_profile_read");
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  for (int k = 0; k < KP1_MLP_PROFILE_SLOTS; ++k) {
    double total_ms = 0.0;
    for (int i = 0; i < m->prof_used[k]; ++i) {
      HIP_TRY(hipEventSynchronize(m->prof[k][i].b));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, m->prof[k][i].a, m->prof[k][i].b));
      total_ms += ms;
    }
    out_launches[k] = m->prof_used[k];
    out_us[k] = m->prof_used[k] > 0 ? (float)(total_ms * 1e3 / m->prof_used[k]) : 0.f;
    m->prof_used[k] = 0;
  }
  return KP1_OK;
}

int kp1_mlp_time_kernels(kp1_mlp* m, const float* obs, int32_t obs_stride, int32_t n, int32_t iters, float* out_ms, double* out_flops,
                         void* stream_) {
  if (!m || !obs || !out_ms || !out_flops || iters <= 0) return fail(KP1_ERR_INVALID, "bad argument to kp1_mlp_time_kernels");
  if (m->K > 1) return fail(KP1_ERR_UNSUPPORTED, "kp1_mlp_time_kernels is not available on population handles");
  if (n <= 0 || n > m->max_batch) return fail(KP1_ERR_INVALID, "n exceeds the workspace max_batch");
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int Hp = m->Hp, INP = m->L.INP;
  const int64_t act_stride = (int64_t)m->max_batch * Hp;
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  rc = launch_forward_layers(m, obs, obs_stride, nullptr, n, stream);  // fills h1/h2 with real activations
  if (rc != KP1_OK) return rc;
  HIP_TRY(hipMemcpyAsync(m->dz2, m->h2, sizeof(float) * 2 * (size_t)act_stride, hipMemcpyDeviceToDevice, stream));
  auto time_it = [&](int which) -> int {
    HIP_TRY(hipEventRecord(e0, stream));
    for (int it = 0; it < iters; ++it) {
      GemmNT g{};
      g.gather = nullptr; g.ldc = Hp; g.strideC = act_stride; g.M = n; g.N = Hp;
      if (which == 0) {
        g.A = m->h1; g.lda = Hp; g.strideA = act_stride; g.W = m->k.w2; g.strideW = (int64_t)Hp * Hp; g.bias = m->k.b2; g.strideBias = Hp;
        g.C = m->h2; g.K = Hp; g.Kreal = Hp;
        if (launch_nt<EPI_BIAS_TANH>(g, stream) != KP1_OK) return KP1_ERR_NO_DEVICE;
      } else if (which == 1) {
        g = backward_nt_args(m, n);
        g.colsum = nullptr;   // this figure is the GEMM without the bias-1 partials
        if (launch_nt<EPI_DTANH>(g, stream) != KP1_OK) return KP1_ERR_NO_DEVICE;
      } else if (which == 2) {
        GemmTN t{};
        t.B = n; t.chunk = tn_chunk_rows(n, (Hp / 128) * (Hp / 128) * 2);
        t.D = m->dz2; t.ldd = Hp; t.strideD = act_stride; t.X = m->h1; t.ldx = Hp; t.strideX = act_stride;
        t.Nload = Hp; t.n_i_tiles = Hp / 128;
        if (launch_tn(m, t, Hp / 128, Hp, m->slab, nullptr, stream) != KP1_OK) return KP1_ERR_NO_DEVICE;
      } else if (which == 3) {
        g.A = obs; g.lda = obs_stride; g.strideA = 0; g.W = m->k.w1p; g.strideW = (int64_t)Hp * INP; g.bias = m->k.b1; g.strideBias = Hp;
        g.C = m->h1; g.K = INP; g.Kreal = kreal(m, obs_stride);
        if (launch_nt<EPI_BIAS_TANH>(g, stream) != KP1_OK) return KP1_ERR_NO_DEVICE;
      } else if (which == 4) {
        // the fused tile kernel on this workspace: rows 0..n of obs, loss inputs = finite scratch values (layer-2 activations)
        FusedArgs fa{};
        fill_fused_head(fa, m, obs, obs_stride, nullptr, n);
        fa.actions = m->h2; fa.old_logp = m->h2 + (int64_t)ACT * n; fa.adv = m->h2 + (int64_t)(ACT + 1) * n; fa.ret = m->h2 + (int64_t)(ACT + 2) * n;
        fa.adv_mode = 3; fa.adv_mean = 0.f; fa.adv_inv_std = 1.f;
        fa.clip_range = 0.2f; fa.vf_coef = 0.5f; fa.inv_count = 1.f / n;
        fa.h1 = m->h1; fa.dz2 = m->dz2; fa.dz1 = m->dz1; fa.act_stride = act_stride; fa.xf = m->xf;
        fa.bslab = m->bslab; fa.hpart = m->hpart; fa.hpart_stride = 10 * Hp + 32;
        if (launch_fused(fa, stream) != KP1_OK) return KP1_ERR_NO_DEVICE;
      } else {
        if (launch_tn_frag(tn_frag_args(m, n), stream) != KP1_OK) return KP1_ERR_NO_DEVICE;
      }
    }
    HIP_TRY(hipEventRecord(e1, stream));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    out_ms[which] = ms / iters;
    return KP1_OK;
  };
  for (int which : {3, 0, 1, 2}) {  // layer 1 first so h1 stays a valid activation for the others
    rc = time_it(which);
    if (rc != KP1_OK) return rc;
  }
  out_ms[4] = out_ms[5] = 0.f;
  out_flops[4] = out_flops[5] = 0.0;
  if (Hp == FU_HP) {  // the fused training path (it rewrites h1 / dz2 / dz1 in fragment-major order, so it runs last)
    for (int which : {4, 5}) {
      rc = time_it(which);
      if (rc != KP1_OK) return rc;
    }
  }
  const double M = n, H = Hp;
  out_flops[0] = 2.0 * 2.0 * M * H * H;
  out_flops[1] = 2.0 * 2.0 * M * H * H;
  out_flops[2] = 2.0 * 2.0 * M * H * H;
  out_flops[3] = 2.0 * 2.0 * M * H * INP;
  if (Hp == FU_HP) {
    out_flops[4] = 2.0 * 2.0 * M * (H * (double)INP + 2.0 * H * H);  // layer 1 + layer 2 + activation backward (heads: < 3 % more)
    out_flops[5] = 2.0 * 2.0 * M * (H * H + H * (double)INP);        // dW2 + dW1
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return KP1_OK;
}

// ---------------------------------------------------------------------------------------------- placement self-check
// Two SPEED assumptions of the update kernels rest on how the hardware places workgroups (never correctness): the training tile holds back
// the workgroups with linear index in [#CUs, 2 #CUs) on the assumption that workgroup k + #CUs lands on the CU of workgroup k (the second tile
// of a CU), and the weight-gradient kernel makes the batch chunk the fast block index on the assumption that block b runs on XCD b % 8.  This
// probe launches a kernel with the training tile's launch shape (grid, block, dynamic LDS, two workgroups per CU), keeps every workgroup resident
// until all have arrived (bounded wait), and records where each one ran.
__global__ void __launch_bounds__(FU_NTH, 2) placement_probe_kernel(unsigned int* __restrict__ where, unsigned int* __restrict__ arrived, unsigned int total) {
  extern __shared__ float lds[];
  if (threadIdx.x == 0) {
    const unsigned int hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);      // HW_REG_HW_ID: wave, SIMD, pipe, CU, SH, SE
    const unsigned int xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);     // HW_REG_XCC_ID[3:0]
    const unsigned int linear = blockIdx.x + gridDim.x * blockIdx.z;
    where[linear] = (xcc << 16) | (((hw >> 13) & 7u) << 8) | (((hw >> 12) & 1u) << 4) | ((hw >> 8) & 15u);   // XCD | SE | SH | CU
    lds[0] = 0.f;
    __hip_atomic_fetch_add(arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < total && wall_clock64() - t0 < 200000ull) __builtin_amdgcn_s_sleep(8);   // <= 2 ms
  }
  __syncthreads();
}

int kp1_mlp_placement_check(int32_t device, int32_t n_rows, int32_t* out, void* stream_) {
  // out[0] workgroups, out[1] pairs (k, k + #CUs) probed, out[2] pairs on the same CU, out[3] workgroups on the XCD of workgroup (index % 8),
  // out[4] #CUs, out[5] distinct CUs used, out[6] workgroups that arrived while the probe waited, out[7] distinct XCDs among workgroups 0..7
  if (!out || n_rows <= 0) return fail(KP1_ERR_INVALID, "bad argument to kp1_mlp_placement_check");
  HIP_TRY(hipSetDevice(device));
  hipStream_t stream = (hipStream_t)stream_;
  int n_cus = 0;
  HIP_TRY(hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, device));
  const dim3 grid((n_rows + FU_BM - 1) / FU_BM, 1, 2);
  const unsigned int total = grid.x * grid.z;
  if ((int)total > 2 * n_cus) return fail(KP1_ERR_UNSUPPORTED, "placement probe: the grid must be resident at once");
  unsigned int* dev = nullptr;
  HIP_TRY(hipMalloc(&dev, sizeof(unsigned int) * (total + 1)));
  HIP_TRY(hipMemsetAsync(dev, 0, sizeof(unsigned int) * (total + 1), stream));
  const size_t bytes = sizeof(float) * FU_LDS_FLOATS;
  HIP_TRY(hipFuncSetAttribute((const void*)placement_probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  hipLaunchKernelGGL(placement_probe_kernel, grid, dim3(FU_NTH), bytes, stream, dev, dev + total, total);
  std::vector<unsigned int> host(total + 1);
  hipError_t e = hipMemcpyAsync(host.data(), dev, sizeof(unsigned int) * (total + 1), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  (void)hipFree(dev);
  HIP_TRY(e);
  int pairs = 0, same = 0, rr = 0;
  std::vector<unsigned int> seen;
  for (unsigned int k = 0; k < total; ++k) {
    if ((host[k] >> 16) == (host[k & 7u] >> 16)) ++rr;      // same XCD as the first workgroup of its residue class (the XCD numbering itself is the hardware's)
    if (k + (unsigned)n_cus < total) {
      ++pairs;
      if (host[k] == host[k + n_cus]) ++same;
    }
    bool fresh = true;
    for (unsigned int v : seen) fresh = fresh && v != host[k];
    if (fresh) seen.push_back(host[k]);
  }
  int xcds = 0;
  for (unsigned int a = 0; a < 8 && a < total; ++a) {
    bool fresh = true;
    for (unsigned int b = 0; b < a; ++b) fresh = fresh && (host[a] >> 16) != (host[b] >> 16);
    xcds += fresh ? 1 : 0;
  }
  out[0] = (int)total; out[1] = pairs; out[2] = same; out[3] = rr; out[4] = n_cus; out[5] = (int)seen.size(); out[6] = (int)host[total]; out[7] = xcds;
  return KP1_OK;
}

#ifdef KP1_CLK_TRACE
int kp1_debug_clk_trace(unsigned long long* out) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(kp1_clk_buf), sizeof(unsigned long long) * 2 * 1024 * 4));
  return KP1_OK;
}
#endif

#ifdef KP1_NT_TRACE
int kp1_debug_nt_trace(unsigned long long* out, int clear) {
  HIP_TRY(hipDeviceSynchronize());
  if (out) HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(kp1_nt_trace_buf), sizeof(unsigned long long) * KP1_TRACE_SLOTS * KP1_TRACE_WGS));
  if (clear) {
    std::vector<unsigned long long> z(KP1_TRACE_SLOTS * KP1_TRACE_WGS, 0ull);
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(kp1_nt_trace_buf), z.data(), sizeof(unsigned long long) * z.size()));
  }
  return KP1_OK;
}
#endif

int kp1_mlp_adam_step(kp1_mlp* m, float* params, float* grad, float* exp_avg, float* exp_avg_sq, float lr, float eps, float max_grad_norm,
                      int32_t step, int32_t zero_grad, void* stream_) {
  if (!m || !params || !grad || !exp_avg || !exp_avg_sq) return fail(KP1_ERR_INVALID, "bad argument to kp1_mlp_adam_step");
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = m->L.total;
  // zero_grad & 2: the caller did not touch grad since kp1_mlp_loss_grad (single GPU), so the sum-of-squares partials
  // the finalize kernel left are the norm of exactly this gradient and the extra reduction launch is skipped
  const bool fused_norm = (zero_grad & 2) && m->n_finalize_blocks > 0;
  const double* norm_partials = fused_norm ? m->partials + 2 * N_PARTIALS : m->partials + N_PARTIALS;
  const int n_norm_partials = fused_norm ? m->n_finalize_blocks : N_PARTIALS;
  ProfScope ps(m, KP1_MLP_PROFILE_ADAM, stream);
  const bool pop = m->K > 1;
  const unsigned r_partials = pop ? (unsigned)PARTIALS_STRIDE : 0u;   // per-replica strides and the hyper-parameter table: population forms only
  const bool line_on = m->hparams_on && !pop;   // a K = 1 handle with its line on: the population forms of the Adam kernels, grid.y = 1
  const float* hparams = m->hparams_on ? (const float*)m->hparams_dev : (const float*)nullptr;
  if (!fused_norm)
    hipLaunchKernelGGL(pop ? sumsq_partials_kernel<true> : sumsq_partials_kernel<false>, dim3(N_PARTIALS, m->K), dim3(256), 0, stream, grad, n,
                       m->partials + N_PARTIALS, r_partials);
  zero_grad = 0;  // gradients are overwritten by the next finalize; nothing to clear
  // step <= 0: use the device-resident counter that kp1_mlp_loss_grad's finalize kernel increments (graph-replay safe)
  const int host_step = step > 0 ? step : 1;
  const float bc1 = 1.f - std::pow(0.9f, (float)host_step);
  const float bc2 = 1.f - std::pow(0.999f, (float)host_step);
  Packed kfmt = m->k;
  const bool frag_only = m->fused && m->Hp == FU_HP;
  kfmt.formats = frag_only ? PACK_FRAG : (PACK_SLAB | PACK_FRAG);
  m->last_params = params;
  if (frag_only) m->slab_stale = true;
  const dim3 grid((unsigned)((n + ADAM_BLOCK - 1) / ADAM_BLOCK), m->K);
  if (m->gate_on) {
    auto* kernel = pop || line_on ? adam_gated_kernel<true> : adam_gated_kernel<false>;
    KP1_LAUNCH(kernel, grid, dim3(ADAM_BLOCK), 0, stream, params, grad, exp_avg, exp_avg_sq, n, norm_partials, n_norm_partials, step > 0 ? step : 0,
               (const int*)m->step_dev, lr, eps, max_grad_norm, bc1, std::sqrt(bc2), zero_grad, r_partials, hparams, m->L, kfmt,
               (const kp1_kl_gate*)m->gate_dev);
  } else {
    auto* kernel = pop || line_on ? adam_kernel<true> : adam_kernel<false>;
    KP1_LAUNCH(kernel, grid, dim3(ADAM_BLOCK), 0, stream, params, grad, exp_avg, exp_avg_sq, n, norm_partials, n_norm_partials, step > 0 ? step : 0,
               (const int*)m->step_dev, lr, eps, max_grad_norm, bc1, std::sqrt(bc2), zero_grad, r_partials, hparams, m->L, kfmt);
  }
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}

int kp1_mlp_set_kl_gate(kp1_mlp* m, const double* target_kl_host, int32_t n, void* stream_) {
  static_assert(sizeof(kp1_kl_gate) == 32 && offsetof(kp1_kl_gate, stopped) == 8 && offsetof(kp1_kl_gate, stop_kl) == 24, "kp1_kl_gate layout");
  if (!m) return fail(KP1_ERR_INVALID, "NULL argument to kp1_mlp_set_kl_gate");
  if (n != 0 && !target_kl_host) return fail(KP1_ERR_INVALID, "NULL argument to kp1_mlp_set_kl_gate");
  if (n != 0 && n != m->K) return fail(KP1_ERR_INVALID, "kp1_mlp_set_kl_gate needs one target per replica (n = K), or n = 0 to clear the gate");
  if (n != 0 && m->actor_extra_host != 0)
    return fail(KP1_ERR_UNSUPPORTED, "a KL gate is not covered on a handle whose actor tensors have taken extra steps (KP1_MLP_OPT_ACTOR_EXTRA_STEPS)");
  if (n != 0 && !finalize_gate_layout_ok(m->L)) return fail(KP1_ERR_UNSUPPORTED, "the loss statistics of this layout do not share one finalize block");
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(stream, &cap));
  if (cap != hipStreamCaptureStatusNone) return fail(KP1_ERR_INVALID, "kp1_mlp_set_kl_gate cannot run while the stream is being captured");
  const int K = m->K;
  if (n == 0) {
    if (!m->gate_on) return KP1_OK;
    std::vector<int> lines((size_t)K * STEP_DEV_INTS);
    HIP_TRY(hipMemcpyAsync(lines.data(), m->step_dev, sizeof(int) * lines.size(), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int r = 1; r < K; ++r)
      if (lines[(size_t)r * STEP_DEV_INTS + CNT_STEP] != lines[CNT_STEP])
        return fail(KP1_ERR_INVALID, "the replicas' Adam step counts differ: the gate cannot be cleared back to one shared count");
    m->gate_on = false;
    return KP1_OK;
  }
  std::vector<kp1_kl_gate> rec((size_t)K);
  for (int r = 0; r < K; ++r) {
    const double t = target_kl_host[r];
    rec[r] = kp1_kl_gate{};
    rec[r].threshold = (t > 0.0 && std::isfinite(t)) ? 1.5 * t : std::numeric_limits<double>::infinity();   // NaN fails t > 0
  }
  HIP_TRY(hipMemcpyAsync(m->gate_dev, rec.data(), sizeof(kp1_kl_gate) * (size_t)K, hipMemcpyHostToDevice, stream));
  if (!m->gate_on)   // from one shared count to one per replica
    for (int r = 1; r < K; ++r)
      HIP_TRY(hipMemcpyAsync(m->step_dev + r * STEP_DEV_INTS, m->step_dev, sizeof(int) * STEP_DEV_INTS, hipMemcpyDeviceToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  m->gate_on = true;
  return KP1_OK;
}

int kp1_mlp_kl_gate_arm(kp1_mlp* m, void* stream_) {
  if (!m) return fail(KP1_ERR_INVALID, "NULL argument to kp1_mlp_kl_gate_arm");
  if (!m->gate_on) return fail(KP1_ERR_INVALID, "kp1_mlp_kl_gate_arm: no KL gate is set on the handle");
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  hipLaunchKernelGGL(kl_gate_arm_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, m->gate_dev, m->K);
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}

int kp1_mlp_kl_gate_read(kp1_mlp* m, kp1_kl_gate* out_host, int32_t* out_steps, void* stream_) {
  if (!m) return fail(KP1_ERR_INVALID, "NULL argument to kp1_mlp_kl_gate_read");
  if (!m->gate_on) return fail(KP1_ERR_INVALID, "kp1_mlp_kl_gate_read: no KL gate is set on the handle");
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int K = m->K;
  std::vector<int> lines((size_t)K * STEP_DEV_INTS);
  if (out_host) HIP_TRY(hipMemcpyAsync(out_host, m->gate_dev, sizeof(kp1_kl_gate) * (size_t)K, hipMemcpyDeviceToHost, stream));
  if (out_steps) HIP_TRY(hipMemcpyAsync(lines.data(), m->step_dev, sizeof(int) * lines.size(), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (out_steps)
    for (int r = 0; r < K; ++r) out_steps[r] = lines[(size_t)r * STEP_DEV_INTS + CNT_STEP];
  return KP1_OK;
}

int kp1_mlp_anchor_loss_grad(kp1_mlp* m, const float* obs, int32_t obs_stride, const int64_t* idx, int32_t n, const float* teacher_actions,
                             float loss_weight, float* grad_out, float* loss_out, void* stream_) {
  if (!m || !obs || !teacher_actions || !grad_out || !loss_out) return fail(KP1_ERR_INVALID, "NULL argument to kp1_mlp_anchor_loss_grad");
  if (m->gate_on) return fail(KP1_ERR_UNSUPPORTED, "the teacher-anchor step is not covered while a KL gate is set on the handle (it reads the shared step count)");
  if (m->K == 1 && m->hparams_on)
    return fail(KP1_ERR_UNSUPPORTED, "the teacher-anchor step is not covered while a K = 1 handle reads a hyper-parameter line (its K = 1 kernels take scalars)");
  int rc = check_batch_args(m, n, obs_stride);
  if (rc != KP1_OK) return rc;
  if (m->Hp != 128) return fail(KP1_ERR_UNSUPPORTED, "the teacher-anchor step runs on the layer-wise kernels: hidden must be 64 or 128");
  const bool pop = m->K > 1;
  if (pop && !idx) return fail(KP1_ERR_INVALID, "population handles gather their rows through idx [K][n]");
  const int n_blocks = (int)((m->L.total + 255) / 256);
  if (n_blocks > ANCHOR_PARTIALS) return fail(KP1_ERR_INVALID, "parameter vector too large for the anchor sum-of-squares partials");
  rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  constexpr int Hp = 128;
  const int64_t act_stride = (int64_t)m->max_batch * Hp;
  const int hpart_stride = 10 * Hp + 32;
  const int64_t hpart_rep = (int64_t)(m->max_batch / 32) * hpart_stride;
  rc = launch_forward_layers(m, obs, obs_stride, idx, n, stream);
  if (rc != KP1_OK) return rc;
  AnchorHeadArgs a{};
  a.h2 = m->h2; a.strideH = act_stride; a.n = n;
  a.w3 = m->k.w3; a.b3 = m->k.b3;
  a.idx = idx; a.teacher = teacher_actions;
  a.dcoef = loss_weight * 2.f / (float)(ACT * n); a.lcoef = loss_weight / (float)(ACT * n);
  a.dz2 = m->dz2; a.hpart = m->hpart; a.hpart_stride = hpart_stride;
  a.r_act = (unsigned)(2 * act_stride); a.r_hpart = (unsigned)hpart_rep;
  {
    const dim3 hgrid((n + HEAD_ROWS - 1) / HEAD_ROWS, m->K);
    const size_t hbytes = sizeof(float) * (HEADS * Hp + HEAD_ROWS * 8 + 48 + HEAD_ROWS * (Hp + 4));
    auto* kernel = pop ? head_anchor_kernel<Hp, true> : head_anchor_kernel<Hp, false>;
    hipLaunchKernelGGL(kernel, hgrid, dim3(256), hbytes, stream, a);
  }
  // dZ1 = (dZ2 W2) * (1 - h1^2) and the bias-1 partials, then dW2 and dW1: kp1_mlp_loss_grad's launches (the value net's are all zeros)
  rc = launch_nt<EPI_DTANH>(backward_nt_args(m, n), stream);
  if (rc != KP1_OK) return rc;
  int s2_n = 0, s1_n = 0;
  rc = launch_layer_wgrads(m, obs, obs_stride, idx, n, &s2_n, &s1_n, stream);
  if (rc != KP1_OK) return rc;
  AnchorFinalizeArgs fa{};
  FinalizeArgs& f = fa.f;
  fill_finalize(f, m, n, s2_n, s1_n, grad_out);
  f.sumsq = m->anchor_partials;
  f.r_sumsq = (unsigned)ANCHOR_PARTIALS;
  f.step_counter = m->step_dev;
  fa.loss_out = loss_out;
  hipLaunchKernelGGL(pop ? anchor_finalize_kernel<true> : anchor_finalize_kernel<false>, dim3(n_blocks, m->K), dim3(256), 0, stream, fa);
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}

int kp1_mlp_anchor_adam_step(kp1_mlp* m, float* params, float* grad, float* exp_avg, float* exp_avg_sq, float lr, float eps, float max_grad_norm,
                             int32_t step, void* stream_) {
  if (!m || !params || !grad || !exp_avg || !exp_avg_sq) return fail(KP1_ERR_INVALID, "NULL argument to kp1_mlp_anchor_adam_step");
  if (m->gate_on) return fail(KP1_ERR_UNSUPPORTED, "the teacher-anchor step is not covered while a KL gate is set on the handle (it reads the shared step count)");
  if (m->K == 1 && m->hparams_on)
    return fail(KP1_ERR_UNSUPPORTED, "the teacher-anchor step is not covered while a K = 1 handle reads a hyper-parameter line (its K = 1 kernels take scalars)");
  if (m->Hp != 128) return fail(KP1_ERR_UNSUPPORTED, "the teacher-anchor step runs on the layer-wise kernels: hidden must be 64 or 128");
  const int n_blocks = (int)((m->L.total + 255) / 256);
  if (n_blocks > ANCHOR_PARTIALS) return fail(KP1_ERR_INVALID, "parameter vector too large for the anchor sum-of-squares partials");
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  Packed kfmt = m->k;
  kfmt.formats = PACK_SLAB | PACK_FRAG;
  m->last_params = params;
  const bool pop = m->K > 1;
  hipLaunchKernelGGL(pop ? anchor_adam_kernel<true> : anchor_adam_kernel<false>, dim3(n_blocks, m->K), dim3(ADAM_BLOCK), 0, stream, params, (const float*)grad,
                     exp_avg, exp_avg_sq, (const double*)m->anchor_partials, n_blocks, lr, eps, max_grad_norm, m->L, kfmt, (const int*)m->step_dev, (int)step,
                     pop ? (unsigned)ANCHOR_PARTIALS : 0u, pop && m->hparams_on ? (const float*)m->hparams_dev : (const float*)nullptr);
  hipLaunchKernelGGL(anchor_count_kernel, dim3(1), dim3(1), 0, stream, m->step_dev);
  m->actor_extra_host += 1;
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}

}  // extern "C"

namespace {
// KP1_MLP_OPT_TRAIN_TILE: forward, loss and backward of an Hp = 128 handle in one launch.  `heads` is the HeadArgs block of the layer-wise
// path; the partial buffers are taken from the FinalizeArgs that grad_finalize_kernel will read them through.
// The definition stands behind every other launch site of the file: the kernels are emitted in the order in which they are first named,
// and the ones emitted behind a new kernel move (their pc-relative constant addresses change).
int launch_train_tile(kp1_mlp* m, const HeadArgs& heads, const float* obs, int obs_stride, int chunks, float* grad, hipStream_t stream) {
  const int Hp = m->Hp, INP = m->L.INP;
  TrainTile128Args t{};
  t.h = heads;
  t.h.h2 = nullptr; t.h.dz2 = nullptr; t.h.r_act = 0u;   // the activations stay in LDS
  t.obs = obs; t.obs_stride = obs_stride; t.Kreal = kreal(m, obs_stride);
  fill_layer_weights(t, m);
  t.w2t = m->k.w2t;
  t.n_w1 = (unsigned)(Hp * INP); t.n_w2 = (unsigned)(Hp * Hp); t.n_b = (unsigned)Hp;
  FinalizeArgs f{};
  fill_finalize(f, m, heads.n, chunks, chunks, grad);
  t.slab2 = m->slab; t.s2_ld = f.s2_ld; t.s2_net = f.s2_net; t.s2_chunk = f.s2_chunk;
  t.slab1 = m->slab1; t.s1_ld = f.s1_ld; t.s1_net = f.s1_net; t.s1_chunk = f.s1_chunk;
  t.bslab = m->bslab; t.b_net = f.b_net; t.b_tile = f.b_tile;
  t.r_slab2 = f.r_slab2; t.r_slab1 = f.r_slab1; t.r_bslab = f.r_bslab;
  const bool pop = m->K > 1 || m->hparams_on;   // a K = 1 handle with its hyper-parameter line on runs the population form, grid.y = 1
  auto* kernel = INP == 64 ? (pop ? train_tile128_kernel<64, true> : train_tile128_kernel<64, false>)
                           : (pop ? train_tile128_kernel<128, true> : train_tile128_kernel<128, false>);
  KP1_LAUNCH(kernel, dim3(chunks, m->K, 2), dim3(ES_NTH), 0, stream, t);   // static LDS: no attribute call, capture-safe
  return KP1_OK;
}
}  // namespace

extern "C" int kp1_mlp_hparams_store(kp1_mlp* m, const kp1_replica_hparams* host, int32_t n, void* stream) {
  if (!m || !host) return fail(KP1_ERR_INVALID, "NULL argument to kp1_mlp_hparams_store");
  if (n != m->K) return fail(KP1_ERR_INVALID, "kp1_mlp_hparams_store needs one entry per replica (n = K)");
  for (int r = 0; r < n; ++r) {
    const kp1_replica_hparams& h = host[r];
    for (float v : {h.learning_rate, h.adam_eps, h.max_grad_norm, h.clip_range, h.ent_coef, h.vf_coef})
      if (!std::isfinite(v)) return fail(KP1_ERR_INVALID, "kp1_mlp_hparams_store: hyper-parameters must be finite");
  }
  if (m->K == 1 && m->bf16x3) return fail(KP1_ERR_UNSUPPORTED, "the bf16x3 weight-gradient experiment has no hyper-parameter line form (kp1_mlp_hparams_store)");
  int rc = mlp_check_device(m);
  if (rc != KP1_OK) return rc;
  // the entries travel as kernel arguments (kp1_mlp_line.hip's hparams_store_kernel): no copy from caller memory is queued, `host` is free on
  // return and nothing waits for the stream
  rc = kp1::mlp_line_store(m->hparams_dev, reinterpret_cast<const float*>(host), n * HP_FIELDS, (hipStream_t)stream);
  if (rc != KP1_OK) return rc;
  m->hparams_on = true;
  return KP1_OK;
}
#endif  // KP1_MLP_LINE_TU
