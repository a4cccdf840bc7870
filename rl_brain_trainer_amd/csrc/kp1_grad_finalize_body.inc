// Body of grad_finalize_kernel and grad_finalize_gated_kernel (kp1_mlp.hip): one text, included by both.  In scope at the include: the kernel
// arguments `a_` (FinalizeArgs) and `n_main`, the template argument POP, `constexpr bool GATE` and `gate` (kp1_kl_gate*, the replicas' records;
// a constant nullptr in the ungated kernel, where every GATE branch is discarded and the kernel compiles to what it was without them).
  const FinalizeArgs a = POP ? finalize_args_replica(a_, blockIdx.y) : a_;
  const ParamLayout& L = a.L;
  __shared__ double sq[4];
  __shared__ float red[8][32];
  float gval = 0.f;
  double gsq = 0.0;
  if ((int)blockIdx.x < n_main) {
    const int64_t j = (int64_t)(blockIdx.x * 256u + threadIdx.x);
    const int64_t per2 = (int64_t)L.H * L.H / 4, per1 = (int64_t)L.H * L.IN / 4;
    if (j < 2 * (per2 + per1)) {
      const float* src;
      int64_t stride, dst;
      int n;
      if (j < 2 * per2) {
        const int net = j >= per2;
        const unsigned rem = (unsigned)(j - net * per2), q4 = (unsigned)(L.H / 4), row = rem / q4, c4 = rem - row * q4;   // 32-bit: see pack_one
        src = a.slab2 + net * a.s2_net + (int64_t)row * a.s2_ld + 4 * c4;
        stride = a.s2_chunk; n = a.s2_n;
        dst = (net ? L.v_w2 : L.p_w2) + (int64_t)row * L.H + 4 * c4;
      } else {
        const int64_t k = j - 2 * per2;
        const int net = k >= per1;
        const unsigned rem = (unsigned)(k - net * per1), q4 = (unsigned)(L.IN / 4), row = rem / q4, c4 = rem - row * q4;
        src = a.slab1 + net * a.s1_net + (int64_t)row * a.s1_ld + 4 * c4;
        stride = a.s1_chunk; n = a.s1_n;
        dst = (net ? L.v_w1 : L.p_w1) + (int64_t)row * L.IN + 4 * c4;
      }
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      int c = 0;
      // the kernel is bound by memory round trips, not bandwidth: 32 partials (one whole dW2 element at the default batch split) are in
      // flight before the first add; the adds keep the chunk order 0, 1, 2, ... whatever the unroll
      for (; c + 32 <= n; c += 32) {
        f32x4 v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = *reinterpret_cast<const f32x4*>(src + (int64_t)(c + u) * stride);
#pragma unroll
        for (int u = 0; u < 32; ++u) s += v[u];
      }
      for (; c + 16 <= n; c += 16) {
        f32x4 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = *reinterpret_cast<const f32x4*>(src + (int64_t)(c + u) * stride);
#pragma unroll
        for (int u = 0; u < 16; ++u) s += v[u];
      }
      for (; c + 8 <= n; c += 8) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4*>(src + (int64_t)(c + u) * stride);
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
      }
      for (; c < n; ++c) s += *reinterpret_cast<const f32x4*>(src + (int64_t)c * stride);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a.grad[dst + q] = s[q];
        gsq += (double)s[q] * (double)s[q];
      }
    }
    if constexpr (!GATE) {   // (the gated form leaves both to the block of the statistics, below)
    if (a.step_counter && blockIdx.x == 0 && threadIdx.x == 0) {  // read by the adam kernel that follows, with the bias corrections of the new count
      const int step = a.step_counter[CNT_STEP] + 1;
      a.step_counter[CNT_STEP] = step;
      adam_record_write(a.step_counter, step, a.step_counter[CNT_EXTRA]);
    }
    if (a.stats && blockIdx.x == 0 && threadIdx.x == 3) {  // entropy of the state-independent diagonal Gaussian
      float ent = 0.f;
      for (int k = 0; k < ACT; ++k) ent += 0.5f + LOG_SQRT_2PI + a.log_std[k];
      a.stats[2] += ent;
    }
    }
  } else {
    const int64_t n_wide = finalize_wide_count(L);
    const int el = threadIdx.x & 31, strand = threadIdx.x >> 5;
    const int64_t e = (int64_t)(blockIdx.x - n_main) * 32 + el;
    // elements n_wide .. n_wide+2 are the three loss sums (policy, value, kl), not gradients
    const bool is_grad = e < n_wide, is_stat = !is_grad && e < n_wide + 3;
    PartialSrc s{};
    int64_t flat = 0;
    if (is_grad) {
      flat = finalize_wide_index(L, e);
      s = finalize_source(a, flat);
    } else if (is_stat) {
      s.p = a.hpart + 10 * L.Hp + 15 + (e - n_wide);
      s.stride = a.h_stride; s.n = a.h_n; s.add = 0.f;
    }
    float part = 0.f;
    if (is_grad || is_stat) {
      int c = strand;
      for (; c + 8 * 31 < s.n; c += 8 * 32) {
        float v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = s.p[(int64_t)(c + 8 * u) * s.stride];
#pragma unroll
        for (int u = 0; u < 32; ++u) part += v[u];
      }
      // the rest, eight in flight (written `part += load` per tile it compiles to load, wait, add: one memory round trip per tile); a load
      // past the end reads the strand's last tile and adds +0.0, which leaves the sum as it is
      for (; c < s.n; c += 8 * 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = s.p[(int64_t)min(c + 8 * u, s.n - 1) * s.stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) part += c + 8 * u < s.n ? v[u] : 0.f;
      }
    }
    red[strand][el] = part;
    __syncthreads();
    if (threadIdx.x < 32) {
      float t = red[0][el];
#pragma unroll
      for (int k = 1; k < 8; ++k) t += red[k][el];
      if constexpr (!GATE) {
      if (is_grad) {
        gval = t + s.add;
        a.grad[flat] = gval;
      } else if (is_stat && a.stats) {
        const int k = (int)(e - n_wide);
        a.stats[k == 2 ? 3 : k] += t * a.inv_count;  // single writer
      }
      } else {
        // The gated form.  The three loss sums and the entropy term belong to lanes n_wide % 32 .. + 3 of this wave (one block:
        // finalize_gate_layout_ok), so the lane of the KL sum can decide for all four: they read `stopped` in one load, in front of its store.
        kp1_kl_gate* const rec = gate + (POP ? blockIdx.y : 0u);
        const int stopped_before = rec->stopped;
        if (is_grad) {
          gval = t + s.add;
          a.grad[flat] = gval;
        } else if (is_stat && a.stats && !stopped_before) {
          const int k = (int)(e - n_wide);
          a.stats[k == 2 ? 3 : k] += t * a.inv_count;  // single writer
        }
        if (e == n_wide + 3 && a.stats && !stopped_before) {   // entropy of the state-independent diagonal Gaussian
          float ent = 0.f;
          for (int k = 0; k < ACT; ++k) ent += 0.5f + LOG_SQRT_2PI + a.log_std[k];
          a.stats[2] += ent;
        }
        if (e == n_wide + 2) {   // the lane of the KL sum: the only writer of the record and of the replica's step line
          // the product on its own, never contracted into the sum above: the float a freshly zeroed stats_out[3] receives
          float kl;
          asm("v_mul_f32 %0, %1, %2" : "=v"(kl) : "v"(t), "v"(a.inv_count));
          const int seen = rec->n_seen;
          if (!stopped_before) {
            rec->n_counted += 1;
            if ((double)kl > rec->threshold) {
              rec->stopped = 1;
              rec->stop_index = seen;
              rec->stop_kl = kl;
            } else {   // the step the Adam launch behind this one takes, with its bias corrections
              int* line = a_.step_counter + (POP ? blockIdx.y : 0u) * (unsigned)STEP_DEV_INTS;
              const int step = line[CNT_STEP] + 1;
              line[CNT_STEP] = step;
              adam_record_write(line, step, line[CNT_EXTRA]);
            }
          }
          rec->n_seen = seen + 1;
        }
      }
    }
  }
  // block sum of squares: shuffles inside a wave, the four wave sums through LDS (fixed order) -- one barrier instead of nine
  double w = gsq + (double)gval * (double)gval;
  for (int off = 32; off > 0; off >>= 1) w += __shfl_xor(w, off);
  if ((threadIdx.x & 63) == 0) sq[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) a.sumsq[blockIdx.x] = ((sq[0] + sq[1]) + sq[2]) + sq[3];
