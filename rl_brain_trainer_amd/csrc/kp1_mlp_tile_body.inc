// Body of mlp_tile_kernel and mlp_tile_line_kernel (kp1_mlp_tile.inc): one text, included by both.  In scope at the include: the kernel
// argument `a` (FusedArgs), TRAIN, K1S, ENV and SPLIT (template arguments in mlp_tile_kernel, constants in the line form), `constexpr bool LINE`
// and `line` (const float*: the handle's hyper-parameter line, kp1_replica_hparams of replica 0; a constant nullptr in mlp_tile_kernel, whose
// LINE branches are discarded -- that kernel compiles to what it was before the text moved here).
  static_assert(!(TRAIN && ENV), "the env step rides on the inference tile only");
  static_assert(TRAIN || !SPLIT, "split planes are written by the training tile");
  // LINE: clip_range and vf_coef come from the line, not from FusedArgs -- kernarg pointer + constant offset, read at kernel entry in front
  // of any divergence (a uniform load once per workgroup, as head_args_replica does); FU_CLIP_RANGE / FU_VF_COEF name the source in the loss
  float line_clip = 0.f, line_vf = 0.f;
  if constexpr (LINE) {
    line_clip = line[HP_CLIP];
    line_vf = line[HP_VF];
  }
#define FU_CLIP_RANGE (LINE ? line_clip : a.clip_range)
#define FU_VF_COEF (LINE ? line_vf : a.vf_coef)
  constexpr bool EVAL = ENV >= 3 && ENV <= 6, EPISODE = ENV == 5 || ENV == 6;
  constexpr int EVAL_MODE = (ENV == 3 || ENV == 5) ? KP1_MODE_APPROACH : KP1_MODE_DOCK;
  constexpr int NW = FU_NW, CB = FU_CB, BM = FU_BM, NTH = FU_NTH, CW = 32 * CB;
  constexpr int INP = K1S * FU_BKS, FU_XP = INP + 4, GS_L2 = K1S, GS_BW = K1S + 8, GS_END = K1S + 16;
  constexpr int KG = FU_BKS / 8, NB = CB * KG;  // B-operand float4 per lane per stage
  // 8-deep k groups of layer 1 that hold observation columns: 56 floats = 7 of the 8 groups of the 64-deep layout, 80 (route keys) = 10 of 16;
  // the rest is zero padding on both operands, and its MFMAs (1.4 % of a training tile's, 19 % of layer 1's with the route keys) are skipped
  constexpr int L1_REAL_GROUPS = K1S == 2 ? (KP1_MLP_IN + 7) / 8 : (KP1_MLP_IN_ROUTE + 7) / 8;
  extern __shared__ float lds[];
  float* bufA = lds;
  float* bufB = bufA + BM * FU_AP;
  float* w3s = bufB + BM * FU_AP;      // [8][256] head weights, resident
  float* dotred = w3s + HEADS * FU_HP; // [4 k-quarters][BM rows][8 outs]
  float* dout = dotred + 4 * BM * 8;   // [BM][8] d loss / d (mean_0..6 | value)
  float* wsum = dout + BM * 8;         // [NW waves][24] per-wave sums
  float* misc = wsum + NW * 24;        // [0] adv mean, [1] adv 1/std

  const int z = (int)blockIdx.z + a.net_base;
  const int m0 = blockIdx.x * BM, slot = blockIdx.x;  // 32-row partial slot
  // the wave index is wave-uniform: taking it through readfirstlane puts it (and every address derived from it) into scalar registers, so
  // the weight-fragment loads use the scalar-base + 32-bit lane offset form and need no 64-bit vector address arithmetic
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // this lane's slice of every stage: [stage][col block = wave*CB + c][kg][lane][4]
  const unsigned lane_off = (unsigned)lane * 16u;   // bytes
  const char* __restrict__ W1F = reinterpret_cast<const char*>(a.k.w1f + (int64_t)z * K1S * FU_STAGE + wave * NB * 64 * 4);
  const char* __restrict__ W2F = reinterpret_cast<const char*>(a.k.w2f + (int64_t)z * 8 * FU_STAGE + wave * NB * 64 * 4);
  const char* __restrict__ W2TF = reinterpret_cast<const char*>(a.k.w2tf + (int64_t)z * 8 * FU_STAGE + wave * NB * 64 * 4);

  // global stage gs: K1S stages of layer 1, then 8 of layer 2, then 8 backward (W2^T); register ring of three stages
  f32x4 bf[3][NB];
#define FU_BLOAD(gs)                                                                                    \
  if ((gs) < GS_END) {                                                                                  \
    const char* p_ = (gs) < GS_L2 ? W1F + (gs) * (FU_STAGE * 4) : ((gs) < GS_BW ? W2F + ((gs) - GS_L2) * (FU_STAGE * 4) : W2TF + ((gs) - GS_BW) * (FU_STAGE * 4)); \
    _Pragma("unroll") for (int q = 0; q < NB; ++q) bf[(gs) % 3][q] = fu_wload(p_, q * 1024 + lane_off); \
  }
  f32x16 acc[CB];
  // accumulators start at the layer bias of their column (a lane's 16 elements of a column block share one column): the bias add costs
  // no vector instruction in the epilogue -- vector instructions are paid in MFMA time on this hardware (see kp_tanh)
#define FU_INIT_ACC(bias)                                                                               \
  _Pragma("unroll") for (int c = 0; c < CB; ++c)                                                        \
    _Pragma("unroll") for (int e = 0; e < 16; ++e) acc[c][e] = (bias)[c];
  // one GEMM of KT stages starting at global stage GS0; A rows from `abuf` (pitch ap).  The sched_barrier after the
  // weight loads keeps them at the top of the stage: left alone, the scheduler sinks every load down to its first use two
  // stages later ("load; s_waitcnt vmcnt(0); mfma"), which turns the prefetch ring into a chain of exposed L2 round trips.
#ifdef KP1_TR_HEADS   // developer trace: slots 7..10 stamp the sub-phases of the head / loss phase instead of the G2 stages
#define KP1_TR_G2(slot)
#define KP1_TR_HD(slot) KP1_TR(slot)
#else
#define KP1_TR_G2(slot) KP1_TR(slot)
#define KP1_TR_HD(slot)
#endif
#ifdef KP1_FU_NOMFMA   // developer experiment (tools/ab_build.sh): everything but the matrix instructions
#define FU_MFMA(acc_, a_, b_) acc_[0] += (a_) * (b_);
#else
#define FU_MFMA(acc_, a_, b_) acc_ = __builtin_amdgcn_mfma_f32_32x32x2f32(a_, b_, acc_, 0, 0, 0);
#endif
#ifdef KP1_FU_NOTANH
#define FU_TANH(x) (x)
#else
#define FU_TANH(x) kp_tanh(x)
#endif
// (reading the A fragments of stage s+1 before the MFMAs of stage s was measured slower and removed: DESIGN.md 4.1)
#define FU_GEMM(abuf, ap, KT, GS0)                                                                      \
  {                                                                                                     \
    const float* as = (abuf) + (lane & 31) * (ap) + 4 * (lane >> 5);                                     \
    _Pragma("unroll") for (int s = 0; s < (KT); ++s) {                                                  \
      FU_BLOAD((GS0) + s + 2)                                                                           \
      __builtin_amdgcn_sched_barrier(0);                                                                \
      f32x4 av[KG];                                                                                     \
      _Pragma("unroll") for (int kg = 0; kg < KG; ++kg)                                                 \
        av[kg] = *reinterpret_cast<const f32x4*>(as + s * FU_BKS + kg * 8);                              \
      _Pragma("unroll") for (int kg = 0; kg < KG; ++kg)                                                 \
        if (!((GS0) == 0 && s * KG + kg >= L1_REAL_GROUPS))   /* layer 1: the k groups past the observation width are zero padding */ \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                   \
          _Pragma("unroll") for (int c = 0; c < CB; ++c)                                                \
            FU_MFMA(acc[c], av[kg][i], bf[((GS0) + s) % 3][c * KG + kg][i])                              \
      __builtin_amdgcn_sched_barrier(0);                                                                \
      if ((GS0) == GS_L2) { KP1_TR_G2(7 + s) }                                                          \
    }                                                                                                   \
  }
  // element e of block c of this lane's accumulators sits at (row, col) of the BM x 256 tile
#define FU_ROW(e) (((e) & 3) + 8 * ((e) >> 2) + 4 * (lane >> 5))
#define FU_COL(c) (wave * CW + (c) * 32 + (lane & 31))
  // accumulator blocks -> k8-fragment-major rows m0 .. m0+BM-1 of dst (256 columns): elements 4g .. 4g+3 of a block are one float4 of
  // that order, so every store instruction is one coalesced 1 KB wave store and nothing goes through LDS
#ifdef KP1_FU_NOSTORE
#define FU_STORE_ACC(dst)
#else
#define FU_STORE_ACC(dst)                                                                               \
  _Pragma("unroll") for (int c = 0; c < CB; ++c)                                                        \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                     \
      const f32x4 v_ = {acc[c][4 * g], acc[c][4 * g + 1], acc[c][4 * g + 2], acc[c][4 * g + 3]};        \
      *reinterpret_cast<f32x4*>((dst) + ((int64_t)((m0 >> 3) + g) * (FU_HP / 32) + wave * CB + c) * 256 + lane * 4) = v_; \
    }
#endif
  // [r3 experiment] accumulator blocks -> the three bf16 planes (two 16-row fragments per 32-row block)
#define FU_STORE_ACC_SPLIT(dst, plane)                                                                  \
  if constexpr (SPLIT) {                                                                               \
    _Pragma("unroll") for (int c = 0; c < CB; ++c)                                                      \
      _Pragma("unroll") for (int f = 0; f < 2; ++f) {                                                   \
        float v8_[8];                                                                                   \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) v8_[j] = acc[c][8 * f + j];                       \
        store_split3((dst) + (int64_t)z * ((plane) / 2), (plane), (int64_t)(m0 >> 4) + f, FU_HP / 32, wave * CB + c, lane, split3(v8_)); \
      }                                                                                                 \
  }
  // [r3 experiment] LDS tile [BM][pitch] (C columns) -> the three bf16 planes; `zoff` selects the net's half of a plane (0 for X)
#define FU_STORE_FRAG_SPLIT(tile, pitch, dst, plane, zoff, C)                                           \
  if constexpr (SPLIT) {                                                                               \
    _Pragma("unroll") for (int q = wave; q < (BM / 16) * ((C) / 32); q += NW) {                         \
      const int f_ = q / ((C) / 32), cb_ = q % ((C) / 32);                                              \
      const float* t_ = (tile) + (16 * f_ + 4 * (lane >> 5)) * (pitch) + 32 * cb_ + (lane & 31);        \
      float v8_[8];                                                                                     \
      _Pragma("unroll") for (int j = 0; j < 8; ++j) v8_[j] = t_[(8 * (j >> 2) + (j & 3)) * (pitch)];    \
      store_split3((dst) + (zoff), (plane), (int64_t)(m0 >> 4) + f_, (C) / 32, cb_, lane, split3(v8_));  \
    }                                                                                                   \
  }
  // LDS tile [BM][pitch] (C columns) -> k8-fragment-major rows m0 .. m0+BM-1 of dst: one coalesced 1 KB store per
  // (8-row group, 32-column block), spread over the waves.  All BM rows are written (rows >= n hold zeros or are
  // multiplied by zeros downstream), so the consumer never sees stale data inside its last 8-row group.
#ifdef KP1_FU_NOSTORE
#define FU_STORE_FRAG(tile, pitch, dst, C)
#else
#define FU_STORE_FRAG(tile, pitch, dst, C)                                                              \
  _Pragma("unroll") for (int q = wave; q < (BM / 8) * ((C) / 32); q += NW) {                            \
    const int g_ = q / ((C) / 32), cb_ = q % ((C) / 32);                                                \
    const float* t_ = (tile) + (8 * g_ + 4 * (lane >> 5)) * (pitch) + 32 * cb_ + (lane & 31);           \
    f32x4 v_;                                                                                           \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) v_[i] = t_[i * (pitch)];                              \
    *reinterpret_cast<f32x4*>((dst) + ((int64_t)((m0 >> 3) + g_) * ((C) / 32) + cb_) * 256 + lane * 4) = v_; \
  }
#endif

  // ------------------------------------------------------------------------------------------------ prologue
  KP1_TR(0)
  if (TRAIN) { KP1_CLK(0, 0) }
  // 32-row tiles: the first two workgroups of a CU (dispatch order k and k + #CUs) start together and, left alone, run every phase in
  // lockstep -- two tiles in an epilogue at once leave the matrix pipes idle.  Holding the second one back by more than the longest
  // non-GEMM phase keeps them apart for the whole tile (measured at M = 8192: 0 us -> 54.8, 6 -> 52.9, 12 -> 51.2 us per launch).
  if (TRAIN && a.stagger_ticks > 0) {
    const int linear = blockIdx.x + gridDim.x * blockIdx.z;
    if (linear >= a.n_cus && linear < 2 * a.n_cus) {
      const unsigned long long t0_ = wall_clock64();
      while (wall_clock64() - t0_ < (unsigned long long)a.stagger_ticks) __builtin_amdgcn_s_sleep(16);
    }
  }
  // EPISODE: this lane's episode (wave 0 keeps it current), the env step in hand, the tile's alive count after it
  bool ep_alive = false;
  int ep_step = a.ev.step, ep_n_alive = 0;
  unsigned ep_zero = 0;
  if constexpr (EPISODE) {
    ep_alive = lane < BM && m0 + lane < a.n && a.ev.b.flags[m0 + lane] != 0;
    if (!__ballot(ep_alive)) return;   // the same answer in all four waves: nothing has written a flag yet
  }
  do {   // (not indented: one pass for every instantiation but the episode forms)
  FU_BLOAD(0)
  FU_BLOAD(1)
  __builtin_amdgcn_sched_barrier(0);
  {
    constexpr int XQ = INP / 4, X_LOADS = BM * XQ / NTH;  // 2 (or 4) float4 per thread
    constexpr int W3_LOADS = HEADS * FU_HP / 4 / NTH;     // head weights: 2 (or 1) float4 per thread
    static_assert(X_LOADS >= 1 && X_LOADS * NTH == BM * XQ && W3_LOADS >= 1 && W3_LOADS * NTH == HEADS * FU_HP / 4, "prologue loads must tile the workgroup");
    int64_t xrow[X_LOADS];
    f32x4 xv[X_LOADS], w3v[W3_LOADS];
#pragma unroll
    for (int j = 0; j < X_LOADS; ++j) {
      const int m = min(m0 + (tid + NTH * j) / XQ, a.n - 1);
      xrow[j] = a.idx ? a.idx[m] : (int64_t)m;
    }
#pragma unroll
    for (int j = 0; j < X_LOADS; ++j) {
      const int k = 4 * ((tid + NTH * j) % XQ);
      xv[j] = *reinterpret_cast<const f32x4*>(a.obs + xrow[j] * a.obs_stride + (k < a.Kreal ? k : 0));
    }
    // head weights -> LDS (resident)
#pragma unroll
    for (int j = 0; j < W3_LOADS; ++j) w3v[j] = *reinterpret_cast<const f32x4*>(a.k.w3 + 4 * (tid + NTH * j));
#pragma unroll
    for (int j = 0; j < X_LOADS; ++j) {
      const int f = tid + NTH * j, row = f / XQ, k = 4 * (f % XQ);
      const float keep = (m0 + row < a.n && k < a.Kreal) ? 1.f : 0.f;
      *reinterpret_cast<f32x4*>(bufB + row * FU_XP + k) = xv[j] * keep;
    }
#pragma unroll
    for (int j = 0; j < W3_LOADS; ++j) *reinterpret_cast<f32x4*>(w3s + 4 * (tid + NTH * j)) = w3v[j];
  }
  if (TRAIN && z == 0 && wave == 0) {  // advantage normalisation statistics of this minibatch (policy workgroups only)
    float mean = 0.f, inv_std = 1.f;
    if (a.adv_mode == 1) {
      double ps = 0.0, pss = 0.0;
      for (int k = lane; k < a.n_adv_partials; k += 64) {
        ps += a.adv_partials[2 * k];
        pss += a.adv_partials[2 * k + 1];
      }
      for (int off = 32; off > 0; off >>= 1) {
        ps += __shfl_xor(ps, off);
        pss += __shfl_xor(pss, off);
      }
      const double mu = ps / a.n;
      const double var = a.n > 1 ? fmax((pss - a.n * mu * mu) / (a.n - 1), 0.0) : 0.0;
      mean = (float)mu;
      inv_std = (float)(1.0 / (sqrt(var) + 1e-8));
    } else if (a.adv_mode == 2) {
      mean = a.adv_stats[0];
      inv_std = a.adv_stats[1];
    } else if (a.adv_mode == 3) {
      mean = a.adv_mean;
      inv_std = a.adv_inv_std;
    }
    if (lane == 0) {
      misc[0] = mean;
      misc[1] = inv_std;
    }
  }
  // this thread's layer biases and its loss-row gather index -> registers
  float bias1[CB], bias2[CB];
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    bias1[c] = a.k.b1[z * FU_HP + FU_COL(c)];
    bias2[c] = a.k.b2[z * FU_HP + FU_COL(c)];
  }
  // loss phase mapping: thread = (row tid>>3, head output tid&7); a wave covers 8 rows
  const int l_row = tid >> 3, l_out = tid & 7;
  const bool l_ok = m0 + l_row < a.n;
  const int64_t l_src = a.idx ? a.idx[min(m0 + l_row, a.n - 1)] : (int64_t)min(m0 + l_row, a.n - 1);
  __syncthreads();
  KP1_TR(1)
  // (experiment mode writes ONLY the bf16 planes: the fp32 k8-fragment copies feed the exact weight-gradient kernel, which then does not run)
  constexpr bool fp32_out = !SPLIT;
  if (TRAIN && z == 0 && fp32_out) { FU_STORE_FRAG(bufB, FU_XP, a.xf, INP) }
  if (TRAIN && z == 0) { FU_STORE_FRAG_SPLIT(bufB, FU_XP, a.sp_xf, a.sp_plane_x, (int64_t)0, INP) }

  // ------------------------------------------------------------------------------------------------ G1: h1
  FU_INIT_ACC(bias1)
  FU_GEMM(bufB, FU_XP, K1S, 0)
#pragma unroll
  for (int c = 0; c < CB; ++c)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      acc[c][e] = FU_TANH(acc[c][e]);
      bufA[FU_ROW(e) * FU_AP + FU_COL(c)] = acc[c][e];
    }
  if (TRAIN && fp32_out) { FU_STORE_ACC(a.h1 + z * a.act_stride) }  // h1 tile -> HBM for the dW2 GEMM; nothing waits on these stores
  if (TRAIN) { FU_STORE_ACC_SPLIT(a.sp_h1, a.sp_plane) }
  __syncthreads();
  KP1_TR(2)
  // per-row loss inputs (gather index arrived during G1): in flight under G2, consumed in the head phase
  float l_act = 0.f, l_old = 0.f, l_adv = 0.f, l_ret = 0.f, l_b3 = a.k.b3[l_out], l_ls = a.k.log_std[l_out < ACT ? l_out : 0];
  if (TRAIN) {
    if (z == 0) {
      if (l_out < ACT) l_act = a.actions[l_src * ACT + l_out];
      l_old = a.old_logp[l_src];
      l_adv = a.adv[l_src];
    } else {
      l_ret = a.ret[l_src];
    }
  } else if (z == 0 && a.noise && l_ok && l_out < ACT) {
    l_act = a.noise[l_src * ACT + l_out];  // N(0,1) draw of this (row, action dimension)
  }

  // ------------------------------------------------------------------------------------------------ G2: h2
  FU_INIT_ACC(bias2)
  FU_GEMM(bufA, FU_AP, 8, GS_L2)
  // bufB (X) was last read in G1, which every wave left before the barrier above
#pragma unroll
  for (int c = 0; c < CB; ++c)
#pragma unroll
    for (int e = 0; e < 16; ++e) bufB[FU_ROW(e) * FU_AP + FU_COL(c)] = FU_TANH(acc[c][e]);
  __syncthreads();
  KP1_TR(3)

  // ------------------------------------------------------------------------------------------------ heads + loss
  {
    // partial dot products: lane = (row, k half), wave = k quarter; the W3 reads are LDS broadcasts
    const int row = lane & 31, kq = wave, part = kq * 2 + (lane >> 5);
    const float* hrow = bufB + row * FU_AP + part * 32;
    f32x4 hv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) hv[q] = *reinterpret_cast<const f32x4*>(hrow + 4 * q);
    auto dot = [&](int o) {
      const float* w = w3s + o * FU_HP + part * 32;
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + 4 * q);
        s = fmaf(hv[q].x, wv.x, s);
        s = fmaf(hv[q].y, wv.y, s);
        s = fmaf(hv[q].z, wv.z, s);
        s = fmaf(hv[q].w, wv.w, s);
      }
      s += __shfl_xor(s, 32);
      if (lane < 32) dotred[(kq * BM + row) * 8 + o] = s;
    };
    if (z == 0) {
#pragma unroll
      for (int o = 0; o < ACT; ++o) dot(o);
    } else {
      dot(7);
    }
  }
  __syncthreads();
  KP1_TR_HD(7)
  if (!TRAIN) {
    // policy.forward tail (SB3 DiagGaussianDistribution): thread = (row, head output)
    const bool mine = z == 0 ? l_out < ACT : l_out == 7;
    float v = 0.f;
    if (mine) {
#pragma unroll
      for (int p = 0; p < 4; ++p) v += dotred[(p * BM + l_row) * 8 + l_out];
      v += l_b3;
    }
    float lp = 0.f;
    if (z == 0) {
      float act = v;
      if (l_ok && l_out < ACT) {
        if (a.mean) a.mean[l_src * ACT + l_out] = v;
        if (a.noise) {
          act = fmaf(expf(l_ls), l_act, v);
          lp = -0.5f * l_act * l_act - l_ls - LOG_SQRT_2PI;
        }
        if (a.action) a.action[l_src * ACT + l_out] = act;
        if (a.clipped) a.clipped[l_src * ACT + l_out] = fminf(fmaxf(act, -1.f), 1.f);
      }
      lp += __shfl_xor(lp, 1);
      lp += __shfl_xor(lp, 2);
      lp += __shfl_xor(lp, 4);
      if (l_ok && l_out == 0 && a.log_prob) a.log_prob[l_src] = lp;
      if constexpr (ENV == 1 || ENV == 2) {
        // the tile's actions -> LDS (dout: [BM][8], idle in inference), then lane r of wave 0 steps env m0 + r; the other waves are done
        dout[l_row * 8 + l_out] = (l_ok && l_out < ACT) ? act : 0.f;    // step_env_lane clips to [-1, 1] itself (arm_kinematic_env.py:214)
        __syncthreads();
        if (wave == 0) {
          const bool live = lane < BM && m0 + lane < a.n;
          float o[KP1_OBS_DIM];
          if (live) step_env_lane<float, ENV == 1 ? KP1_MODE_APPROACH : KP1_MODE_DOCK, false>(a.env, (int64_t)(m0 + lane), dout + lane * 8, o);
          // the tile's observation rows leave as whole-line stores; bufA (h1) was last read in G2, two barriers ago
          store_obs_tile(a.env.obs, (int64_t)m0, min(BM, a.n - m0), o, live, a.env.obs_stride, bufA);
        }
      }
      if constexpr (EVAL) {
        // evaluation step: the clamped mean (the clamp a.clipped gets above) -> LDS, then lane r of wave 0 is episode m0 + r
        dout[l_row * 8 + l_out] = (l_ok && l_out < ACT) ? fminf(fmaxf(v, -1.f), 1.f) : 0.f;
        __syncthreads();
        if (wave == 0) {
          const bool live = lane < BM && m0 + lane < a.n;
          float o[KP1_OBS_DIM];
          int alive_after = 0;
          if (EPISODE ? ep_alive : live) {
            const int64_t i = (int64_t)(m0 + lane) + (EPISODE ? ep_zero : 0u);
            const double an = es_action_norm(dout + lane * 8);
            if constexpr (EPISODE) step_env_lane<float, EVAL_MODE, false>(es_episode_env(a.env, ep_zero), i, dout + lane * 8, o);
            else step_env_lane<float, EVAL_MODE, false>(a.env, i, dout + lane * 8, o);
            // the fields the step has just stored are read back from the handle by the lane that stored them
            alive_after = eval_account_step<float>(a.env.st.real, (int)a.env.st.n, (int)i, a.ev.b, an, a.env.done[i], EPISODE ? ep_step : a.ev.step,
                                                   a.ev.track_ready != 0, a.ev.thr_pos, a.ev.thr_ori, a.ev.thr_act, a.ev.thr_dq, a.ev.confirm);
          } else if (EPISODE && ES_EPISODE_REREADS<EVAL_MODE> && live) {
            // a finished (or never started) episode is not stepped: its row of the tile is its current observation
            const f32x4* src = reinterpret_cast<const f32x4*>(a.env.obs + (int64_t)(m0 + lane) * a.env.obs_stride);
#pragma unroll
            for (int k = 0; k < KP1_OBS_DIM / 4; ++k) {
              const f32x4 v4 = src[k];
              o[4 * k] = v4.x; o[4 * k + 1] = v4.y; o[4 * k + 2] = v4.z; o[4 * k + 3] = v4.w;
            }
          }
          const unsigned long long bal = __ballot(alive_after != 0);
          if constexpr (!EPISODE) {
            if (lane == 0 && bal) atomicAdd(a.ev.b.n_alive, __popcll(bal));
          }
          // the tile's next observations; bufA (h1) was last read in G2, two barriers ago.  This is the step's only write to a.env.obs
          if constexpr (EPISODE && !ES_EPISODE_REREADS<EVAL_MODE>) store_obs_rows(a.env.obs, (int64_t)m0, (unsigned)__ballot(ep_alive), o, a.env.obs_stride, bufA);
          else store_obs_tile(a.env.obs, (int64_t)m0, min(BM, a.n - m0), o, live, a.env.obs_stride, bufA);
          if constexpr (EPISODE) {
            ep_alive = alive_after != 0;
            if (lane == 0) reinterpret_cast<int*>(misc)[2] = __popcll(bal);
          }
        }
        if constexpr (EPISODE) {
          __syncthreads();             // the tile's new observation rows and the alive count, for all four waves
          ep_n_alive = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(misc)[2]);
          ep_zero = (unsigned)ep_n_alive >> 31;   // a count is never negative
        }
      }
    } else if (l_ok && l_out == 7 && a.value) {
      a.value[l_src] = v;
    }
    if constexpr (EPISODE) continue;   // to the loop's condition
    else return;
  }
  {
    const int row_l = l_row, out = l_out;
    const bool ok = l_ok;
    const bool mine = z == 0 ? out < ACT : out == 7;
    float v = 0.f;
    if (mine) {
#pragma unroll
      for (int p = 0; p < 4; ++p) v += dotred[(p * BM + row_l) * 8 + out];
      v += l_b3;
    }
    float zs = 0.f, inv_sd = 1.f, lp = 0.f;
    if (z == 0 && ok && out < ACT) {
      inv_sd = expf(-l_ls);
      zs = (l_act - v) * inv_sd;
      lp = -0.5f * zs * zs - l_ls - LOG_SQRT_2PI;
    }
    lp += __shfl_xor(lp, 1);
    lp += __shfl_xor(lp, 2);
    lp += __shfl_xor(lp, 4);
    float g_logp = 0.f, d = 0.f, pl = 0.f, vl = 0.f, kl = 0.f;
    if (ok && z == 0) {
      const float A = (l_adv - misc[0]) * misc[1];
      const float lr_ = lp - l_old;
      const float ratio = expf(lr_);
      const float rc = fminf(fmaxf(ratio, 1.f - FU_CLIP_RANGE), 1.f + FU_CLIP_RANGE);
      const float s1 = ratio * A, s2 = rc * A;
      // d/dlogp of -min(s1, s2): the unclipped branch carries the gradient unless the clipped one is strictly smaller
      const bool inside = ratio >= 1.f - FU_CLIP_RANGE && ratio <= 1.f + FU_CLIP_RANGE;
      g_logp = (inside || s1 < s2) ? -A * ratio * a.inv_count : 0.f;
      if (out < ACT) {
        d = g_logp * zs * inv_sd;
      } else {
        pl = -fminf(s1, s2);
        kl = (ratio - 1.f) - lr_;
      }
    } else if (ok && out == 7) {
      d = FU_VF_COEF * 2.f * (v - l_ret) * a.inv_count;
      vl = (l_ret - v) * (l_ret - v);
    }
    dout[row_l * 8 + out] = (ok && mine) ? d : 0.f;
    // per-wave sums over this wave's 8 rows (lanes with equal out): bias grads, log_std grads, loss terms
    float gls = (z == 0 && ok && out < ACT) ? g_logp * (zs * zs - 1.f) : 0.f;
    float dsum = (ok && mine) ? d : 0.f;
    float l0 = pl, l1 = vl, l2 = kl;
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) {
      gls += __shfl_xor(gls, off);
      dsum += __shfl_xor(dsum, off);
      l0 += __shfl_xor(l0, off);
      l1 += __shfl_xor(l1, off);
      l2 += __shfl_xor(l2, off);
    }
    if (lane < 8) {
      wsum[wave * 24 + out] = dsum;
      wsum[wave * 24 + 8 + out] = gls;
      if (out == 7) {
        wsum[wave * 24 + 16] = l0;
        wsum[wave * 24 + 17] = l1;
        wsum[wave * 24 + 18] = l2;
      }
    }
  }
  KP1_TR_HD(8)
  __syncthreads();
  KP1_TR_HD(9)
  if (tid < 18) {
    // 0..7 head-bias grads, 8..14 log_std grads, 15..17 loss sums (policy, value, kl); each net writes its own
    const int k = tid;
    const int w = k < 8 ? k : (k < 15 ? 8 + (k - 8) : 16 + (k - 15));
    const float v = ((wsum[w] + wsum[24 + w]) + wsum[48 + w]) + wsum[72 + w];   // the four waves, summed in wave order
    const bool pi_slot = (k < 7) || (k >= 8 && k < 15) || k == 15 || k == 17;
    if (pi_slot == (z == 0)) a.hpart[(int64_t)slot * a.hpart_stride + 10 * FU_HP + k] = v;
  }
  {
    // dZ2 = (dOut W3) * (1 - h2^2) in place.  Wave = 64-column range, lane = (column group cg of 4, row group rg): 16 column groups x
    // 4 row groups of 8 rows; the head-weight and bias-2 gradient partials are then summed over the row groups by shuffles -- no LDS, no barrier.
    constexpr int DZ_COLS = FU_HP / NW, DZ_CG = DZ_COLS / 4, DZ_RG = 64 / DZ_CG, DZ_ROWS = 32 / DZ_RG;
    const int cg = lane % DZ_CG, rg = lane / DZ_CG, col = wave * DZ_COLS + 4 * cg;
    float* part = a.hpart + (int64_t)slot * a.hpart_stride;
    f32x4 gw[ACT], gb2 = {0.f, 0.f, 0.f, 0.f}, w3c[ACT];
#pragma unroll
    for (int o = 0; o < ACT; ++o) {
      gw[o] = f32x4{0.f, 0.f, 0.f, 0.f};
      w3c[o] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (z == 0) {
#pragma unroll
      for (int o = 0; o < ACT; ++o) w3c[o] = *reinterpret_cast<const f32x4*>(w3s + o * FU_HP + col);
    } else {
      w3c[0] = *reinterpret_cast<const f32x4*>(w3s + 7 * FU_HP + col);
    }
#pragma unroll
    for (int j = 0; j < DZ_ROWS; ++j) {
      const int row = rg * DZ_ROWS + j;
      const f32x4 h = *reinterpret_cast<const f32x4*>(bufB + row * FU_AP + col);
      f32x4 dp = {0.f, 0.f, 0.f, 0.f};
      if (z == 0) {
#pragma unroll
        for (int o = 0; o < ACT; ++o) {
          const float dd = dout[row * 8 + o];
          dp += dd * w3c[o];
          gw[o] += dd * h;
        }
      } else {
        const float dd = dout[row * 8 + 7];
        dp = dd * w3c[0];
        gw[0] += dd * h;
      }
      const f32x4 dz = dp * (1.f - h * h);
      gb2 += dz;
      *reinterpret_cast<f32x4*>(bufB + row * FU_AP + col) = dz;
    }
    auto fold = [&](f32x4 v) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int off = DZ_CG; off < 64; off <<= 1) v[i] += __shfl_xor(v[i], off);
      }
      return v;
    };
    gb2 = fold(gb2);
    if (z == 0) {
#pragma unroll
      for (int o = 0; o < ACT; ++o) {
        const f32x4 t = fold(gw[o]);
        if (rg == 0) *reinterpret_cast<f32x4*>(part + o * FU_HP + col) = t;
      }
      if (rg == 0) *reinterpret_cast<f32x4*>(part + 8 * FU_HP + col) = gb2;
    } else {
      const f32x4 t = fold(gw[0]);
      if (rg == 0) {
        *reinterpret_cast<f32x4*>(part + 7 * FU_HP + col) = t;
        *reinterpret_cast<f32x4*>(part + 9 * FU_HP + col) = gb2;
      }
    }
  }
  KP1_TR_HD(10)
  __syncthreads();  // dZ2 tile complete
  KP1_TR(4)
  if (fp32_out) { FU_STORE_FRAG(bufB, FU_AP, a.dz2 + z * a.act_stride, FU_HP) }
  if (TRAIN) { FU_STORE_FRAG_SPLIT(bufB, FU_AP, a.sp_dz2, a.sp_plane, (int64_t)z * (a.sp_plane / 2), FU_HP) }

  // ------------------------------------------------------------------------------------------------ G3: dZ1
  {
    float zero[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) zero[c] = 0.f;
    FU_INIT_ACC(zero)
  }
  FU_GEMM(bufB, FU_AP, 8, GS_BW)
  // dZ1 = acc * (1 - h1^2) with h1 read back from the positions this lane wrote after G1; column sums of the tile are the bias-1
  // gradient partials of its slot; dZ1 leaves from the registers
  {
    float* __restrict__ bs = a.bslab + ((int64_t)slot * 2 + z) * FU_HP;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      float csum = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float h = bufA[FU_ROW(e) * FU_AP + FU_COL(c)];
        const float v = acc[c][e] * (1.f - h * h);   // rows >= n carry dZ2 = 0, hence 0 here
        csum += v;
        acc[c][e] = v;
      }
      csum += __shfl_xor(csum, 32);
      if (lane < 32) bs[FU_COL(c)] = csum;
    }
  }
  KP1_TR(5)
  if (fp32_out) { FU_STORE_ACC(a.dz1 + z * a.act_stride) }
  FU_STORE_ACC_SPLIT(a.sp_dz1, a.sp_plane)
  KP1_TR(6)
  KP1_CLK(0, 1)
  } while (EPISODE && ep_n_alive != 0 && ep_step++ < a.ev.last_step);
  if constexpr (EPISODE) {
    if (tid == 0 && ep_n_alive) atomicAdd(a.ev.b.n_alive, ep_n_alive);
  }
#undef FU_BLOAD
#undef FU_INIT_ACC
#undef FU_GEMM
#undef FU_MFMA
#undef FU_TANH
#undef FU_ROW
#undef FU_COL
#undef FU_STORE_ACC
#undef FU_STORE_FRAG
#undef FU_STORE_ACC_SPLIT
#undef FU_STORE_FRAG_SPLIT
#undef FU_CLIP_RANGE
#undef FU_VF_COEF
