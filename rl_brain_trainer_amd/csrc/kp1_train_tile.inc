// kp1_train_tile.inc -- forward, PPO loss and backward of a 32-row tile of ONE net in ONE launch, for the layer-wise widths (hidden 64 / 128,
// both in the Hp = 128 layout of struct Packed): KP1_MLP_OPT_TRAIN_TILE.  Included by kp1_mlp.hip inside its anonymous namespace as the last
// kernel file, behind kp1_rollout_run.inc, so that every other kernel keeps its place in the code object (uses es_layer and the ES_* geometry
// of kp1_eval_step.inc, head_dot, HeadArgs / head_args_replica, and the two statement files it shares with head_train_kernel,
// kp1_head_adv_body.inc and kp1_head_loss_body.inc; DESIGN.md sections 28 and 31).
//
// It stands where kp1_mlp_loss_grad launched gemm_nt (layer 1), gemm_nt (layer 2), head_train_kernel, gemm_nt<EPI_DTANH> and two gemm_tn:
// [adv_partials ->] train_tile128 -> grad_finalize.  h1, h2, dZ2 and dZ1 live in LDS only.
//
// grid = (chunk, replica, net), 256 threads = four waves; wave w owns hidden columns [32 w, 32 w + 32), es_layer's decomposition.  The policy
// net and the value net of a row are independent in head_train_kernel's arithmetic (g_logp needs the advantage, the value head needs `ret`),
// so a workgroup carries one net and writes that net's entries only.
//
// Chunking: a chunk is R consecutive 32-row tiles, and R is a function of n alone: R = 1 for every n this kernel serves, n <= TT_MAX_ROWS =
// 2048 rows per replica = 64 chunks, the slab room a handle has per replica.  Larger n takes the layer-wise launches (train_tile_chunks
// returns 0).  With R = 1 a chunk is a tile is a 32-row block of head_train_kernel: chunk c writes slab c of dW2 and of dW1, row c of the
// b1 partials and record c of hpart, each element by one thread with a plain store, and grad_finalize_kernel sums s2_n = s1_n = b_n = h_n =
// chunks of them in chunk order.  Nothing depends on K, the device or the occupancy: a replica computes what a K = 1 handle computes.
// No workgroup waits on another one; no atomics.
//
// What equals the layer-wise launches bit for bit, and why:
//  * h1, h2: es_layer issues gemm_nt_kernel's chain (top of kp1_eval_step.inc); the x tile holds what gemm_nt_kernel's masked loads hold
//    (rows >= n and columns >= Kreal are zero, the gather goes through idx).
//  * heads, loss, dout, the per-wave sums: the text head_train_kernel compiles, at its thread mapping; the four wave slots are summed in
//    its order.  So every hpart entry but the dZ2 column sums is head_train_kernel's expression on equal inputs.
//  * phase 2 (dZ2, head weight gradients, b2 gradients): one thread per hidden column walks the block's rows in order, head_train_kernel's
//    expressions for this net.
// The weight gradients and the b1 gradient are other sums than gemm_tn_kernel's and gemm_nt_kernel's (32 rows per partial, not 64 or more).
//
// Per tile: x gather -> LDS | es_layer<INP> -> h1 | es_layer<128> -> h2 | heads, loss, dout | dZ2 over h2 | dW2 = dZ2^T h1 (MFMA, both
// operands batch-row major in LDS, gemm_tn_kernel's operand form; a wave's 32 x 128 strip) | dZ1 = (dZ2 W2) * (1 - h1^2) from k.w2t over h1,
// its column sums = the b1 partial | dW1 = dZ1^T x.
constexpr int TT_MAX_CHUNKS = 64;                      // slabs per replica (kp1_mlp_create)
constexpr int TT_MAX_ROWS = TT_MAX_CHUNKS * ES_BM;     // R = 1 up to here
// chunks of an n-row minibatch, or 0: the layer-wise launches take it
__host__ __device__ inline int train_tile_chunks(int n) { return n >= 1 && n <= TT_MAX_ROWS ? (n + ES_BM - 1) / ES_BM : 0; }

// (the name's length matters to `check_device_code.py --compare` against the parent: DESIGN.md section 31, code objects)
struct TrainTile128Args {
  HeadArgs h;                          // heads, loss inputs, hyper-parameters, hpart (h2, dz2, strideH unused: they stay in LDS)
  const float* obs; int obs_stride;    // rollout observations; rows are gathered through h.idx (or rows [0, n) when it is NULL, K = 1)
  int Kreal;
  const float *w1, *b1, *w2, *b2, *w3, *b3;   // fill_layer_weights: net 0 of replica 0; net z at + z * n_*, replica r at + r * r_*
  unsigned r_w1, r_w2, r_b, r_w3, r_b3;
  const float* w2t;                    // k-slab major transpose of w2, strides as w2
  unsigned n_w1, n_w2, n_b;
  // the partial buffers as fill_finalize describes them
  float* slab2; int64_t s2_ld, s2_net, s2_chunk;
  float* slab1; int64_t s1_ld, s1_net, s1_chunk;
  float* bslab; int64_t b_net, b_tile;
  unsigned r_slab2, r_slab1, r_bslab;
};

// a wave's strip of D^T X over the tile's 32 batch rows: rows o in [32 wave, +32) of D^T, NCB 32-column blocks of X, stored to P[o][ld].
// v_mfma_f32_32x32x2_f32 with k = two batch rows: lane l carries batch row 2 s + (l >> 5), D column 32 wave + (l & 31) as the A operand and
// X column 32 c + (l & 31) as the B operand; consecutive lanes read consecutive LDS words.
template <int NCB>
__device__ __forceinline__ void tt_wgrad_strip(const float* __restrict__ ds, const float* __restrict__ xs, int xpitch, float* __restrict__ P, int64_t ld,
                                               int wave, int lane) {
  const int half = lane >> 5, l31 = lane & 31;
  const float* dl = ds + half * ES_HPITCH + 32 * wave + l31;
  const float* xl = xs + half * xpitch + l31;
  float dv[ES_BM / 2];
#pragma unroll
  for (int s = 0; s < ES_BM / 2; ++s) dv[s] = dl[2 * s * ES_HPITCH];
#pragma unroll
  for (int c = 0; c < NCB; ++c) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int s = 0; s < ES_BM / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[s], xl[2 * s * xpitch + 32 * c], acc, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int o = 32 * wave + (e & 3) + 8 * (e >> 2) + 4 * half;
      P[(int64_t)o * ld + 32 * c + l31] = acc[e];
    }
  }
}

template <int INP, bool POP>
__global__ void __launch_bounds__(ES_NTH) train_tile128_kernel(const TrainTile128Args t) {
  constexpr int XP = INP + 4;
  __shared__ __attribute__((aligned(16))) float lds[ES_BM * XP + 2 * ES_H_FLOATS + HEADS * ES_HP + HEAD_ROWS * 8 + 84];
  float* xs = lds;                         // [32][INP + 4]
  float* h1s = xs + ES_BM * XP;            // [32][132]: h1, then dZ1
  float* h2s = h1s + ES_H_FLOATS;          // [32][132]: h2, then dZ2
  float* w3s = h2s + ES_H_FLOATS;          // [8][128]
  float* dout = w3s + HEADS * ES_HP;       // [32][8] : d loss / d (mean_0..6, value)
  float* red = dout + HEAD_ROWS * 8;       // [4 waves][20] per-wave partial sums
  float* adv_ms = red + 80;                // [2] (+2 pad)
  static_assert(HEAD_ROWS == ES_BM, "a tile is one 32-row block of head_train_kernel");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned chunk = blockIdx.x, rep = POP ? blockIdx.y : 0u, net = blockIdx.z;
  const HeadArgs a = POP ? head_args_replica(t.h, rep) : t.h;
  const int m0 = (int)chunk * ES_BM;

  // ---- 1. the tile's observation rows, gathered through idx -> LDS; rows past n are clamped and zeroed, columns >= Kreal read column 0 and are zeroed
  {
    // without idx (K = 1) rows [0, n) of obs; a replica's index row holds rows of the shared rollout buffers
    const float* __restrict__ obs = t.obs;
    constexpr int XQ = INP / 4, X_LOADS = ES_BM * XQ / ES_NTH;
    int64_t xrow[X_LOADS];
#pragma unroll
    for (int j = 0; j < X_LOADS; ++j) {
      const int m = min(m0 + (tid + ES_NTH * j) / XQ, a.n - 1);
      xrow[j] = a.idx ? a.idx[m] : (int64_t)m;
    }
    f32x4 xv[X_LOADS];
#pragma unroll
    for (int j = 0; j < X_LOADS; ++j) {
      const int k = 4 * ((tid + ES_NTH * j) % XQ);
      xv[j] = *reinterpret_cast<const f32x4*>(obs + xrow[j] * t.obs_stride + (k < t.Kreal ? k : 0));
    }
#pragma unroll
    for (int j = 0; j < X_LOADS; ++j) {
      const int f = tid + ES_NTH * j, r = f / XQ, k = 4 * (f % XQ);
      const float keep = (m0 + r < a.n && k < t.Kreal) ? 1.f : 0.f;
      *reinterpret_cast<f32x4*>(xs + r * XP + k) = xv[j] * keep;
    }
  }
  for (int k = tid; k < HEADS * ES_HP; k += ES_NTH) w3s[k] = a.w3[k];
#include "kp1_head_adv_body.inc"
  __syncthreads();

  // ---- 2. this net's hidden layers: h1, h2 in LDS
  es_layer<INP>(xs, XP, t.w1 + rep * t.r_w1 + net * t.n_w1, t.b1 + rep * t.r_b + net * t.n_b, h1s, wave, lane);
  __syncthreads();
  es_layer<ES_HP>(h1s, ES_HPITCH, t.w2 + rep * t.r_w2 + net * t.n_w2, t.b2 + rep * t.r_b + net * t.n_b, h2s, wave, lane);
  __syncthreads();

  // ---- 3. heads of this net, PPO loss, dout, per-wave sums (head_train_kernel's text and thread mapping)
  const int row_l = tid >> 3, out = tid & 7;
  const int row = m0 + row_l;
  const bool ok = row < a.n;
  const int64_t src = ok ? (a.idx ? a.idx[row] : (int64_t)row) : 0;
  float v = 0.f;
  if (ok && (out == 7) == (net != 0)) v = head_dot(h2s + row_l * ES_HPITCH, w3s + out * ES_HP, ES_HP) + a.b3[out];
#include "kp1_head_loss_body.inc"
  __syncthreads();
  float* part = a.hpart + (int64_t)chunk * a.hpart_stride;
  if (tid < 18) {
    const int k = tid;  // 0..7 bias grads, 8..14 log_std grads, 15..17 loss sums (policy, value, kl)
    const int slot = k < 8 ? 4 + k : (k < 15 ? 12 + (k - 8) : k - 15);
    const bool value_entry = k == 7 || k == 16;
    if (value_entry == (net != 0)) part[10 * ES_HP + k] = ((red[slot] + red[20 + slot]) + red[40 + slot]) + red[60 + slot];
  }
  // ---- 4. one thread per hidden column: dZ2 = (dOut W3) * (1 - h2^2) over h2, head weight gradients, b2 gradient of this net.
  // head_train_kernel writes 1.f - h * h, dz = t * that and gb2 += dz, and the compiler contracts them to fma(-h, h, 1), a product and
  // fma(factor, t, gb2) (its listing: v_pk_fma_f32 ... 1.0 neg, v_pk_mul_f32, v_pk_fma_f32).  Here the same source form came out otherwise in
  // the value branch (h * h packed into a v_pk_mul_f32 with dv * w, then a subtraction: the b2 gradient differed in the last bit), so the
  // three operations are spelled as that listing has them.  tests/test_train_tile_gpu.py compares the bits.
  const int rows_here = min(HEAD_ROWS, a.n - m0);
  if (tid < ES_HP) {
    const int h = tid;
    if (net == 0) {
      float wcol[ACT], gw[ACT];
#pragma unroll
      for (int o = 0; o < ACT; ++o) {
        wcol[o] = w3s[o * ES_HP + h];
        gw[o] = 0.f;
      }
      float gb2p = 0.f;
      for (int r = 0; r < rows_here; ++r) {
        const float hp = h2s[r * ES_HPITCH + h];
        float dp = 0.f;
#pragma unroll
        for (int o = 0; o < ACT; ++o) {
          const float dd = dout[r * 8 + o];
          dp = fmaf(dd, wcol[o], dp);
          gw[o] = fmaf(dd, hp, gw[o]);
        }
        const float fp = fmaf(-hp, hp, 1.f);
        h2s[r * ES_HPITCH + h] = dp * fp;
        gb2p = fmaf(fp, dp, gb2p);
      }
#pragma unroll
      for (int o = 0; o < ACT; ++o) part[o * ES_HP + h] = gw[o];
      part[8 * ES_HP + h] = gb2p;
    } else {
      const float wv = w3s[7 * ES_HP + h];
      float gwv = 0.f, gb2v = 0.f;
      for (int r = 0; r < rows_here; ++r) {
        const float hv = h2s[r * ES_HPITCH + h];
        const float dv = dout[r * 8 + 7];
        gwv = fmaf(dv, hv, gwv);
        const float fv = fmaf(-hv, hv, 1.f), tv = dv * wv;
        h2s[r * ES_HPITCH + h] = tv * fv;
        gb2v = fmaf(fv, tv, gb2v);
      }
      part[7 * ES_HP + h] = gwv;
      part[9 * ES_HP + h] = gb2v;
    }
    for (int r = rows_here; r < ES_BM; ++r) h2s[r * ES_HPITCH + h] = 0.f;   // rows past n: no gradient
  }
  __syncthreads();

  // ---- 5. dW2 strip of this wave: dZ2^T h1
  tt_wgrad_strip<ES_HP / 32>(h2s, h1s, ES_HPITCH, t.slab2 + rep * t.r_slab2 + chunk * t.s2_chunk + net * t.s2_net, t.s2_ld, wave, lane);
  __syncthreads();   // every wave has read h1

  // ---- 6. dZ1 = (dZ2 W2) * (1 - h1^2) over h1 (es_layer's chain on the transposed weights), and its column sums: the b1 partial of the chunk
  {
    constexpr int KG = ES_HP / 8;
    const int col = 32 * wave + (lane & 31), khalf = 4 * (lane >> 5);
    const float* wl = t.w2t + rep * t.r_w2 + net * t.n_w2 + col * 32 + khalf;
    f32x4 bw[KG];
#pragma unroll
    for (int kg = 0; kg < KG; ++kg) bw[kg] = *reinterpret_cast<const f32x4*>(wl + (kg >> 2) * (ES_HP * 32) + (kg & 3) * 8);
    const float* al = h2s + (lane & 31) * ES_HPITCH + khalf;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int kg = 0; kg < KG; ++kg) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(al + kg * 8);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bw[kg].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bw[kg].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bw[kg].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bw[kg].w, acc, 0, 0, 0);
    }
    float csum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
      const float hv = h1s[r * ES_HPITCH + col];
      const float dz = acc[e] * (1.f - hv * hv);   // rows past n: dZ2 = 0, so dZ1 = 0
      h1s[r * ES_HPITCH + col] = dz;
      csum += dz;
    }
    csum += __shfl_xor(csum, 32);
    if (lane < 32) t.bslab[rep * t.r_bslab + chunk * t.b_tile + net * t.b_net + col] = csum;
  }
  __syncthreads();

  // ---- 7. dW1 strip of this wave: dZ1^T x (the padded columns of x are zero)
  tt_wgrad_strip<INP / 32>(h1s, xs, XP, t.slab1 + rep * t.r_slab1 + chunk * t.s1_chunk + net * t.s1_net, t.s1_ld, wave, lane);
}
