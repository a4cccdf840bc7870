// kp1_mlp_fused.inc -- the weight-gradient GEMMs of the fused PPO update (H = 256): they read the k8-fragment-major activation tiles
// mlp_tile_kernel (kp1_mlp_tile.inc, included before this file) wrote.  Included by kp1_mlp.hip inside its anonymous namespace.
//
// (An 8-wave "uniform" variant with both batch halves and a dW1 unit in one workgroup measured slower in round 2 and was reverted:
// profiles/r02_ab_tn_round1_vs_uniform.log.)

// ---------------------------------------------------------------------------------------------- weight gradients
// dW2[o][i] = sum_b dZ2[b][o] h1[b][i] and dW1[o][i] = sum_b dZ1[b][o] X[b][i] for both nets in ONE launch, reading the
// k8-fragment-major activations the tile kernel wrote: a lane's A operand (column o of dZ) and B operand (column i of h1 / X)
// for four consecutive MFMAs is one float4, one 8-row group of one 32-column block is one coalesced 1 KB wave load, and
// nothing is staged through LDS -- no barrier in the reduction loop, two workgroups per CU.
// A workgroup owns a 64 x 64 tile of dW2 (32 x inp of dW1) over 1/8 (1/16) of the batch and its four waves split those batch rows:
// every wave accumulates the WHOLE tile over its quarter of the rows (wave tile 64 x 64), the four partial tiles are added through LDS
// in wave order (fixed order: bitwise reproducible) and ONE tile leaves the workgroup, as float4 stores into the slabs
// grad_finalize_kernel sums in fixed order: 8 dW2 + 16 dW1 slabs, 6.3 MB per step.  (The round-1 form -- 128 x 128 tiles over 1/32 of
// the batch, 32 partial slabs per weight, 24.6 MB -- was measured slower and removed: DESIGN.md 4.3.)  Every operand column block is read
// by four workgroups; the block index is laid out so that those four run on ONE XCD under the round-robin dispatch (chunk = blockIdx % 8:
// an XCD's 32 + 32 workgroups stream the same 1024 batch rows through its L2 together) -- placement is a speed assumption only, a
// different one costs L2 hits, never correctness.
struct TnFragArgs {
  const float* dz2; const float* h1; const float* dz1; int64_t act_stride;  // [2][rows x 256] k8-fragment major
  const float* xf; int inp;                                                 // [rows x inp], inp = 64 or 128
  float* slab2; int64_t s2_net, s2_chunk;                                    // [chunk][net][256][256]
  float* slab1; int64_t s1_net, s1_chunk;                                    // [chunk][net][256][inp]
  int groups, cg2, n_chunks2, cg1, n_chunks1;
};

template <int RA, int CB>
__device__ __forceinline__ void tn_split_tile(const float* __restrict__ Af, int a_ncb, const float* __restrict__ Bf, int b_ncb, int g_begin, int g_end,
                                              float* __restrict__ out, int out_ld, float* lds) {
  constexpr int SG = 4;  // 8-row groups per register set; two sets alternate (loads of one under the MFMAs of the other)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int per = (max(g_end - g_begin, 0) + 3) >> 2;                      // 8-row groups per wave
  const int gb = min(g_begin + wave * per, g_end), ge = min(gb + per, g_end);
  const int64_t a_gs = (int64_t)a_ncb * 256, b_gs = (int64_t)b_ncb * 256;  // floats per 8-row group
  f32x4 ra[2][SG][RA], rb[2][SG][CB];
  f32x16 acc[RA][CB];
#pragma unroll
  for (int r = 0; r < RA; ++r)
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[r][c][e] = 0.f;
  KP1_TR(12)
  KP1_TR_HW(11)
  if (gb < ge) {   // wave-uniform
    const int g_last = ge - 1;
    // Groups past the end of the range are clamped to its last group and their A operand is multiplied by 0: the loop body
    // has no branch (a conditional MFMA block made the compiler copy all accumulators through v_mov after every group).
    // The multiply is not overhead: with global loads in flight, MFMAs that read the loaded registers directly and issue back
    // to back run at 40-55 ns each instead of 30 (tools/mfma_load_mix.hip, profiles/r01_mfma_load_mix.log); one VALU
    // instruction per MFMA pair restores the pipe rate (an unmasked fast path for full chunks measured 42 us against 29 us).
#define KP1_TNS_LOAD(set, g0)                                                                           \
  _Pragma("unroll") for (int u = 0; u < SG; ++u) {                                                      \
    const int gg_ = min((g0) + u, g_last);                                                              \
    _Pragma("unroll") for (int r = 0; r < RA; ++r) ra[set][u][r] = load16_sc1(Af, lane * 4 + gg_ * a_gs + r * 256); \
    _Pragma("unroll") for (int c = 0; c < CB; ++c) rb[set][u][c] = load16_sc1(Bf, lane * 4 + gg_ * b_gs + c * 256); \
  }
#define KP1_TNS_MFMA(set, g0)                                                                           \
  _Pragma("unroll") for (int u = 0; u < SG; ++u) {                                                      \
    const float keep_ = (g0) + u < ge ? 1.f : 0.f;                                                      \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                       \
      _Pragma("unroll") for (int r = 0; r < RA; ++r)                                                    \
        _Pragma("unroll") for (int c = 0; c < CB; ++c)                                                  \
          acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[set][u][r][i] * keep_, rb[set][u][c][i], acc[r][c], 0, 0, 0); \
  }
    KP1_TNS_LOAD(0, gb)
    for (int g = gb; g < ge; g += 2 * SG) {
      KP1_TNS_LOAD(1, g + SG)
      __builtin_amdgcn_sched_barrier(0);
      KP1_TNS_MFMA(0, g)
      __builtin_amdgcn_sched_barrier(0);
      KP1_TNS_LOAD(0, g + 2 * SG)
      __builtin_amdgcn_sched_barrier(0);
      KP1_TNS_MFMA(1, g + SG)
      __builtin_amdgcn_sched_barrier(0);
    }
#undef KP1_TNS_LOAD
#undef KP1_TNS_MFMA
  }
  KP1_TR(13)
  // the four waves' partial tiles -> LDS [wave][32 RA rows][LDP]; LDP = width + 8 keeps the two half-waves (rows o and o + 4) on disjoint banks
  constexpr int TO = 32 * RA, TI = 32 * CB, LDP = TI + 8, Q = TI / 4;
  float* mine = lds + wave * (TO * LDP);
#pragma unroll
  for (int r = 0; r < RA; ++r)
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int o = r * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        mine[o * LDP + c * 32 + (lane & 31)] = acc[r][c][e];
      }
  __syncthreads();
  KP1_TR(14)
#pragma unroll
  for (int j = 0; j < TO * Q / 256; ++j) {
    const int f = tid + 256 * j, o = f / Q, q = f % Q;
    const float* p0 = lds + o * LDP + 4 * q;
    const f32x4 v = ((*reinterpret_cast<const f32x4*>(p0) + *reinterpret_cast<const f32x4*>(p0 + TO * LDP)) +
                     *reinterpret_cast<const f32x4*>(p0 + 2 * TO * LDP)) + *reinterpret_cast<const f32x4*>(p0 + 3 * TO * LDP);
    store16_sc1(out, (int64_t)o * out_ld + 4 * q, v);
  }
  KP1_TR(15)
}
constexpr int TN_SPLIT_LDS_FLOATS = 4 * 64 * (64 + 8);   // the largest of the three tile shapes: 4 x 64 x 72 (dW2), 4 x 32 x 72, 4 x 32 x 104

__global__ void __launch_bounds__(256, 2) gemm_tn_split_kernel(const TnFragArgs a) {
  extern __shared__ float lds[];
  KP1_CLK(1, 0)
  const int n2 = 32 * a.n_chunks2;
  if ((int)blockIdx.x < n2) {
    // dW2: 2 nets x 4 x 4 tiles of 64 x 64; the chunk is the fast index: chunk == blockIdx % 8 when there are 8 chunks
    const int chunk = blockIdx.x % a.n_chunks2, tile = blockIdx.x / a.n_chunks2;
    const int net = tile >> 4, ot = (tile >> 2) & 3, it = tile & 3;
    const int g0 = chunk * a.cg2, g1 = min(g0 + a.cg2, a.groups);
    float* out = a.slab2 + chunk * a.s2_chunk + net * a.s2_net + (int64_t)(ot * 64) * FU_HP + it * 64;
    tn_split_tile<2, 2>(a.dz2 + net * a.act_stride + (ot * 2) * 256, 8, a.h1 + net * a.act_stride + (it * 2) * 256, 8, g0, g1, out, FU_HP, lds);
  } else {
    // dW1: 2 nets x 8 tiles of 32 x inp, quarter-size workgroups (half the rows of a dW2 chunk each)
    const int id = blockIdx.x - n2;
    const int chunk = id % a.n_chunks1, tile = id / a.n_chunks1;
    const int net = tile >> 3, ot = tile & 7;
    const int g0 = chunk * a.cg1, g1 = min(g0 + a.cg1, a.groups);
    const int inp = a.inp;
    float* out = a.slab1 + chunk * a.s1_chunk + net * a.s1_net + (int64_t)(ot * 32) * inp;
    if (inp == 64)   // uniform per launch
      tn_split_tile<1, 2>(a.dz1 + net * a.act_stride + ot * 256, 8, a.xf, 2, g0, g1, out, 64, lds);
    else   // 80 observation floats in the 128-wide layout: the fourth 32-column block is zero padding that grad_finalize_kernel never reads
      tn_split_tile<1, 3>(a.dz1 + net * a.act_stride + ot * 256, 8, a.xf, 4, g0, g1, out, 128, lds);
  }
  KP1_CLK(1, 1)
}

// ---------------------------------------------------------------------------------------------- [r3 EXPERIMENT] weight gradients on bf16 x 3 operands
// KP1_MLP_OPT_BF16X3_WGRAD (default OFF; `dtype` and `value` of bench.py stay on the exact fp32 kernel above).  The same GEMMs
// dW2 = dZ2^T h1, dW1 = dZ1^T X with both operands pre-split by the PRODUCER (mlp_tile_kernel, split3) into three bf16 pieces x = hi + mid + lo
// (24 significand bits) and six bf16 MFMAs per fp32-grade product block: lo*hi + hi*lo + mid*mid + hi*mid + mid*hi + hi*hi (smallest terms first;
// the dropped mid*lo, lo*mid, lo*lo are below 2^-24 relative), all accumulated in fp32 by v_mfma_f32_32x32x16_bf16.  A 16-row k step of a
// 64 x 64 wave tile is 24 MFMAs x 32 cycles = 768 cycles against 32 x 64 = 2 048 for the fp32 MFMA form, and the loop has no vector
// instruction: splitting in the consumer would cost ~900 cycles of vector time per step, more than the matrix time saved (DESIGN.md 10).
// Decomposition, slabs and the fixed-order combine are those of gemm_tn_split_kernel; a fragment = 16 batch rows.
struct TnBf16Args {
  const unsigned short* dz2; const unsigned short* h1; const unsigned short* dz1; int64_t plane, net;   // [3 planes][2 nets][rows/16][8 cb][64][8]
  const unsigned short* xf; int64_t plane_x; int inp;                                                 // [3 planes][rows/16][inp/32][64][8]
  float* slab2; int64_t s2_net, s2_chunk;
  float* slab1; int64_t s1_net, s1_chunk;
  int frags, cf2, n_chunks2, cf1, n_chunks1;                                                          // 16-row fragments; per-chunk counts
};

// 16 bytes (8 bf16) at base[off] with the cache-policy bits of the exact kernel's operand loads (sc1)
__device__ __forceinline__ bf16x8 tnb_load(const unsigned short* __restrict__ base, int64_t off) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(base), 0, 0x7fffffff, 0x00020000);
  return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, (int)(off * 2), 0, AUX_SC1));
}

template <int RA, int CB>
__device__ __forceinline__ void tn_bf16_tile(const unsigned short* __restrict__ Af, int64_t a_plane, int a_ncb, const unsigned short* __restrict__ Bf, int64_t b_plane,
                                             int b_ncb, int f_begin, int f_end, float* __restrict__ out, int out_ld, float* lds) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int per = (max(f_end - f_begin, 0) + 3) >> 2;                      // fragments per wave
  const int fb = min(f_begin + wave * per, f_end), fe = min(fb + per, f_end);
  const int64_t a_fs = (int64_t)a_ncb * 512, b_fs = (int64_t)b_ncb * 512;  // bf16 elements per fragment (ncb blocks x 64 lanes x 8)
  bf16x8 ra[2][3][RA], rb[2][3][CB];
  f32x16 acc[RA][CB];
#pragma unroll
  for (int r = 0; r < RA; ++r)
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[r][c][e] = 0.f;
  if (fb < fe) {   // wave-uniform
    const int f_last = fe - 1;
#define KP1_TNB_LOAD(set, f0)                                                                           \
  {                                                                                                     \
    const int ff_ = min((f0), f_last);                                                                  \
    _Pragma("unroll") for (int pl = 0; pl < 3; ++pl) {                                                  \
      _Pragma("unroll") for (int r = 0; r < RA; ++r) ra[set][pl][r] = tnb_load(Af, lane * 8 + pl * a_plane + ff_ * a_fs + r * 512); \
      _Pragma("unroll") for (int c = 0; c < CB; ++c) rb[set][pl][c] = tnb_load(Bf, lane * 8 + pl * b_plane + ff_ * b_fs + c * 512); \
    }                                                                                                   \
  }
#define KP1_TNB_MFMA(set)                                                                               \
  _Pragma("unroll") for (int r = 0; r < RA; ++r)                                                        \
    _Pragma("unroll") for (int c = 0; c < CB; ++c) {                                                    \
      acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[set][2][r], rb[set][0][c], acc[r][c], 0, 0, 0);  /* lo  * hi  */ \
      acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[set][0][r], rb[set][2][c], acc[r][c], 0, 0, 0);  /* hi  * lo  */ \
      acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[set][1][r], rb[set][1][c], acc[r][c], 0, 0, 0);  /* mid * mid */ \
      acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[set][0][r], rb[set][1][c], acc[r][c], 0, 0, 0);  /* hi  * mid */ \
      acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[set][1][r], rb[set][0][c], acc[r][c], 0, 0, 0);  /* mid * hi  */ \
      acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[set][0][r], rb[set][0][c], acc[r][c], 0, 0, 0);  /* hi  * hi  */ \
    }
    KP1_TNB_LOAD(0, fb)
    int f = fb;
    for (; f + 1 < fe; f += 2) {
      KP1_TNB_LOAD(1, f + 1)
      __builtin_amdgcn_sched_barrier(0);
      KP1_TNB_MFMA(0)
      __builtin_amdgcn_sched_barrier(0);
      KP1_TNB_LOAD(0, f + 2)
      __builtin_amdgcn_sched_barrier(0);
      KP1_TNB_MFMA(1)
      __builtin_amdgcn_sched_barrier(0);
    }
    if (f < fe) { KP1_TNB_MFMA(0) }   // odd count: the last fragment sits in set 0
#undef KP1_TNB_LOAD
#undef KP1_TNB_MFMA
  }
  // the four waves' partial tiles -> LDS, added in wave order, one tile leaves the workgroup (as tn_split_tile)
  constexpr int TO = 32 * RA, TI = 32 * CB, LDP = TI + 8, Q = TI / 4;
  float* mine = lds + wave * (TO * LDP);
#pragma unroll
  for (int r = 0; r < RA; ++r)
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int o = r * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        mine[o * LDP + c * 32 + (lane & 31)] = acc[r][c][e];
      }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < TO * Q / 256; ++j) {
    const int fq = tid + 256 * j, o = fq / Q, q = fq % Q;
    const float* p0 = lds + o * LDP + 4 * q;
    const f32x4 v = ((*reinterpret_cast<const f32x4*>(p0) + *reinterpret_cast<const f32x4*>(p0 + TO * LDP)) +
                     *reinterpret_cast<const f32x4*>(p0 + 2 * TO * LDP)) + *reinterpret_cast<const f32x4*>(p0 + 3 * TO * LDP);
    store16_sc1(out, (int64_t)o * out_ld + 4 * q, v);
  }
}

__global__ void __launch_bounds__(256, 2) gemm_tn_bf16x3_kernel(const TnBf16Args a) {
  extern __shared__ float lds[];
  const int n2 = 32 * a.n_chunks2;
  if ((int)blockIdx.x < n2) {
    const int chunk = blockIdx.x % a.n_chunks2, tile = blockIdx.x / a.n_chunks2;
    const int net = tile >> 4, ot = (tile >> 2) & 3, it = tile & 3;
    const int f0 = chunk * a.cf2, f1 = min(f0 + a.cf2, a.frags);
    float* out = a.slab2 + chunk * a.s2_chunk + net * a.s2_net + (int64_t)(ot * 64) * FU_HP + it * 64;
    tn_bf16_tile<2, 2>(a.dz2 + net * a.net + (ot * 2) * 512, a.plane, 8, a.h1 + net * a.net + (it * 2) * 512, a.plane, 8, f0, f1, out, FU_HP, lds);
  } else {
    const int id = blockIdx.x - n2;
    const int chunk = id % a.n_chunks1, tile = id / a.n_chunks1;
    const int net = tile >> 3, ot = tile & 7;
    const int f0 = chunk * a.cf1, f1 = min(f0 + a.cf1, a.frags);
    const int inp = a.inp;
    float* out = a.slab1 + chunk * a.s1_chunk + net * a.s1_net + (int64_t)(ot * 32) * inp;
    if (inp == 64)
      tn_bf16_tile<1, 2>(a.dz1 + net * a.net + ot * 512, a.plane, 8, a.xf, a.plane_x, 2, f0, f1, out, 64, lds);
    else
      tn_bf16_tile<1, 3>(a.dz1 + net * a.net + ot * 512, a.plane, 8, a.xf, a.plane_x, 4, f0, f1, out, 128, lds);
  }
}

