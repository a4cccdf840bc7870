// kp1_x_tile_body.inc -- the statements that bring a tile's ES_BM observation rows into LDS as the x tile of layer 1: rows past the replica's
// last and columns >= Kreal read as zero, as gemm_nt_kernel masks them (the loads stay in bounds: the row index is clamped and a masked column
// reads column 0).  Included as text by eval_step_kernel, rollout_step_kernel, route_rollout_step_kernel, route_chain_step_kernel,
// rollout_run_kernel and rollout_value_kernel, each inside a braced block after its own prologue, which declares
//   X_INP, X_PITCH (constexpr int: the layer-1 width and the LDS pitch of the x tile, ES_INP / ES_XP or INP / G::XP),
//   obs (const float*, row 0 of the replica; __restrict__ where nothing of the launch writes the rows, plain in the looped and in-place forms),
//   x_n, x_stride, x_kreal (int: rows of the replica, row pitch, columns that are read), m0, tid (int), xs (float*, the LDS tile).
// One text, so the copies cannot drift; text and not a call, see DESIGN section 28.
  constexpr int XQ = X_INP / 4, X_LOADS = ES_BM * XQ / ES_NTH;
  f32x4 xv[X_LOADS];
#pragma unroll
  for (int j = 0; j < X_LOADS; ++j) {
    const int f = tid + ES_NTH * j, k = 4 * (f % XQ);
    const int m = min(m0 + f / XQ, x_n - 1);
    xv[j] = *reinterpret_cast<const f32x4*>(obs + (int64_t)m * x_stride + (k < x_kreal ? k : 0));
  }
#pragma unroll
  for (int j = 0; j < X_LOADS; ++j) {
    const int f = tid + ES_NTH * j, r = f / XQ, k = 4 * (f % XQ);
    const float keep = (m0 + r < x_n && k < x_kreal) ? 1.f : 0.f;
    *reinterpret_cast<f32x4*>(xs + r * X_PITCH + k) = xv[j] * keep;
  }
