// Body of adam_kernel and adam_gated_kernel (kp1_mlp.hip): one text, included by both.  In scope at the include: the kernel arguments, the
// template argument POP, `constexpr bool GATE` and `gate` (const kp1_kl_gate*; a constant nullptr in the ungated kernel, whose GATE branch is
// discarded).
  // (argument order: what the loads and the norm need stands in front of the two structs, which are read behind the reduction)
  __shared__ float scale_s;
  if constexpr (GATE) {   // a replica whose gate has stopped leaves before any store; the others step on their own line of the counts
    const unsigned rep = POP ? blockIdx.y : 0u;
    if (gate[rep].stopped) return;   // uniform: the whole launch of this replica
    cnt += rep * (unsigned)STEP_DEV_INTS;
  }
  // the counts and the record (kp1_mlp::step_dev, uniform loads, none of them behind a branch): host_step > 0 is the caller's step count, with
  // bc1 / bc2_sqrt its corrections; otherwise the count is the device's and the corrections are the record's
  const int dev_step = cnt[CNT_STEP], extra = cnt[CNT_EXTRA];
  const int step = host_step > 0 ? host_step : dev_step;
  const int rec_step = cnt[REC_STEP], rec_extra = cnt[REC_EXTRA];
  const float rec_bc1 = __int_as_float(cnt[REC_BC]), rec_bc2_sqrt = __int_as_float(cnt[REC_BC + 1]);
  const float rec_bc1_a = __int_as_float(cnt[REC_BC + 2]), rec_bc2_sqrt_a = __int_as_float(cnt[REC_BC + 3]);
  const Packed k = POP ? packed_replica(k_, L, blockIdx.y) : k_;
  if constexpr (POP) {
    const unsigned o = blockIdx.y * (unsigned)n;
    p += o; g += o; m += o; v += o;
    partials += blockIdx.y * r_partials;
    if (hparams) {   // replica blockIdx.y's entry of the hyper-parameter table (uniform load at kernel entry); same arithmetic below
      const float* e = hparams + blockIdx.y * (unsigned)HP_FIELDS;
      lr = e[HP_LR];
      eps = e[HP_EPS];
      max_norm = e[HP_MAX_NORM];
    }
  }
  // this thread's elements: their loads do not depend on the norm, so they go out first and share one memory round trip with the
  // step count and the norm partials below (the kernel is a chain of round trips: it moves 2.6 MB)
  const int64_t i0 = ((int64_t)blockIdx.x * ADAM_BLOCK + threadIdx.x) * VEC;
  float g_in[VEC], m_in[VEC], v_in[VEC], p_in[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int64_t il = i0 + j < n ? i0 + j : n - 1;
    g_in[j] = g[il]; m_in[j] = m[il]; v_in[j] = v[il]; p_in[j] = p[il];
  }
  double s = 0.0;
  if (threadIdx.x < 64) s = norm_partials_sum(partials, n_partials);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);
    scale_s = max_norm > 0.f ? fminf(max_norm / (norm + 1e-6f), 1.f) : 1.f;
  }
  // torch.optim.Adam keeps one step count per tensor: the actor tensors (policy_net.*, action_net.*) have taken `extra`
  // more steps than the rest when a teacher-anchor side loss updates them between rollouts (route/teacher_anchor.py:68-87)
  float bc1_a, bc2_sqrt_a;
  if (host_step <= 0 && rec_step == step && rec_extra == extra) {   // the launch that advanced the count left the corrections (uniform branch)
    bc1 = rec_bc1; bc2_sqrt = rec_bc2_sqrt; bc1_a = rec_bc1_a; bc2_sqrt_a = rec_bc2_sqrt_a;
  } else {   // a count the host set since, or the caller's
    if (host_step <= 0) adam_bias((float)step, bc1, bc2_sqrt);
    adam_bias_actor((float)step, extra, bc1, bc2_sqrt, bc1_a, bc2_sqrt_a);
  }
  __syncthreads();
  const float scale = scale_s;
  float pn[VEC], mn[VEC], vn[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int64_t i = i0 + j;
    const bool actor = extra != 0 && ((i >= L.p_w1 && i < L.v_w1) || (i >= L.a_w && i < L.c_w));
    const float b1 = actor ? bc1_a : bc1, b2 = actor ? bc2_sqrt_a : bc2_sqrt;
    const float gi = g_in[j] * scale;
    mn[j] = 0.9f * m_in[j] + 0.1f * gi;
    vn[j] = 0.999f * v_in[j] + 0.001f * gi * gi;
    const float denom = sqrtf(vn[j]) / b2 + eps;
    pn[j] = p_in[j] - (lr / b1) * (mn[j] / denom);
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int64_t i = i0 + j;
    if (i < n) {
      m[i] = mn[j]; v[i] = vn[j]; p[i] = pn[j];
      pack_one(i, pn[j], L, k);
      if (zero_grad) g[i] = 0.f;
    }
  }
