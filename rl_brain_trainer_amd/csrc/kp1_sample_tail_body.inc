// kp1_sample_tail_body.inc -- the stochastic action heads of a row tile and head_infer_kernel's sampling tail: thread = (row = t / 8,
// out = t % 8); head `out` of the row is head_dot over its h2 plus the bias; act = fmaf(expf(ls), nz, v) is stored unclipped, its clamp goes
// to the row's lane through `acts`; lp = -0.5f nz nz - ls - LOG_SQRT_2PI per action lane and 0 for lane 7, then the three __shfl_xor sums over
// the 8-lane group, in head_infer_kernel's order.  Rows past the replica's last carry v = lp = clipped = 0 and store nothing.
// Included as text by rollout_step_kernel, route_rollout_step_kernel and rollout_run_kernel, each inside a braced block after its own
// prologue, which declares
//   fw (const RolloutStepArgs, the forward's fields: a copy of the kernel's by-value argument, which the compiler dissolves, or a reference
//   where the kernel already reads its argument through one; a NEW reference to a kernel argument is not transparent, DESIGN section 28),
//   w3, b3 (const float* __restrict__, the replica's head weights and biases),
//   tail_off (const int64_t: rows between slice 0 and this step's slice of action / noise / log_prob; 0 in the one-step kernels),
//   TAIL_STORES_CLIPPED (constexpr bool) and tail_clipped (float*: where the route step reads its caller's action; nullptr without the flag),
//   row, out (int), ok (bool: the row exists), rep (unsigned), env0 (int64_t), h2s, acts (float*, LDS).
// One text, so the copies cannot drift; text and not a call, see DESIGN section 28.
  float v = 0.f;
  if (ok && out < ACT) v = head_dot(h2s + row * ES_HPITCH, w3 + out * ES_HP, ES_HP) + b3[out];
  float lp = 0.f, clipped = 0.f;
  if (ok && out < ACT) {
    const int64_t e = (tail_off + env0 + row) * ACT + out;
    const float ls = fw.log_std[rep * fw.r_b3 + out];
    const float nz = fw.noise[e];
    const float act = fmaf(expf(ls), nz, v);
    lp = -0.5f * nz * nz - ls - LOG_SQRT_2PI;
    fw.action[e] = act;
    clipped = fminf(fmaxf(act, -1.f), 1.f);
    if constexpr (TAIL_STORES_CLIPPED) tail_clipped[e] = clipped;
  }
  acts[row * 8 + out] = clipped;
  lp += __shfl_xor(lp, 1);
  lp += __shfl_xor(lp, 2);
  lp += __shfl_xor(lp, 4);
  if (ok && out == 0 && fw.log_prob) fw.log_prob[tail_off + env0 + row] = lp;
