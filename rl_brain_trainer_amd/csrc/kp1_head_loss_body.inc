// kp1_head_loss_body.inc -- the PPO loss of a 32-row block at thread = (row = t / 8, out = t % 8): the Gaussian log-prob of the stored action
// under head values `v`, the clipped-surrogate gradient g_logp, d loss / d (mean_0..6, value) into dout, and the per-wave partial sums of the
// head-bias gradients, the log_std gradients and the three loss terms into red ([wave 0..3][20] = 3 loss sums, pad, 8 bias grads at +4,
// 7 log_std grads at +12): shuffles inside the wave, the site sums the four wave slots in a fixed order after its barrier.
// Included as text by head_train_kernel and train_tile128_kernel, each after its own prologue, which declares
//   a (const HeadArgs, the replica's), adv_ms, dout, red (float*, LDS; adv_ms already published), row_l, out (int), ok (bool: the row exists),
//   src (int64_t: the row's index into the rollout buffers, 0 when !ok), v (float: head `out` of the row, 0 when !ok).
// A site that carries one net hands v = 0 for the other net's heads and stores only its own net's entries: the policy entries (d for
// out < 7, gls, pl, kl) do not read v of out 7, and the value entries (d for out 7, vl) read nothing else of the row but `ret`.
// One text, so the copies cannot drift; text and not a call, see DESIGN section 28.
  // Gaussian log-prob of the stored action under the current policy
  float z = 0.f, inv_sd = 1.f, lp = 0.f;
  if (ok && out < ACT) {
    const float ls = a.log_std[out];
    inv_sd = expf(-ls);
    z = (a.actions[src * ACT + out] - v) * inv_sd;
    lp = -0.5f * z * z - ls - LOG_SQRT_2PI;
  }
  lp += __shfl_xor(lp, 1);
  lp += __shfl_xor(lp, 2);
  lp += __shfl_xor(lp, 4);
  float g_logp = 0.f, d = 0.f, pl = 0.f, vl = 0.f, kl = 0.f;
  if (ok) {
    const float old = a.old_logp[src];
    const float A = (a.adv[src] - adv_ms[0]) * adv_ms[1];
    const float lr_ = lp - old;
    const float ratio = expf(lr_);
    const float rc = fminf(fmaxf(ratio, 1.f - a.clip_range), 1.f + a.clip_range);
    const float s1 = ratio * A, s2 = rc * A;
    // d/dlogp of -min(s1, s2): the unclipped branch carries the gradient unless the clipped one is strictly smaller
    const bool inside = ratio >= 1.f - a.clip_range && ratio <= 1.f + a.clip_range;
    g_logp = (inside || s1 < s2) ? -A * ratio * a.inv_count : 0.f;
    if (out < ACT) {
      d = g_logp * z * inv_sd;                           // d loss / d mean_out
    } else {
      const float R = a.ret[src];
      d = a.vf_coef * 2.f * (v - R) * a.inv_count;       // d loss / d value
      vl = (R - v) * (R - v);
      pl = -fminf(s1, s2);
      kl = (ratio - 1.f) - lr_;
    }
  }
  dout[row_l * 8 + out] = ok ? d : 0.f;
  // per-block sums over rows of: d loss/d log_std_out, d loss/d head bias_out, loss terms.  Lanes with equal (t & 7) hold
  // the same `out`: reduce inside the wave by shuffles, across the 4 waves through per-wave LDS slots summed in a fixed order.
  float gls = (ok && out < ACT) ? g_logp * (z * z - 1.f) : 0.f;
  gls += __shfl_xor(gls, 8);
  gls += __shfl_xor(gls, 16);
  gls += __shfl_xor(gls, 32);
  float dsum = ok ? d : 0.f;
  dsum += __shfl_xor(dsum, 8);
  dsum += __shfl_xor(dsum, 16);
  dsum += __shfl_xor(dsum, 32);
  // per-wave partials in LDS, combined in a fixed order below (no float atomics: bitwise reproducible run to run).
  // red layout: [wave 0..3][20] = 3 loss sums, pad, 8 bias grads at +4, 7 log_std grads at +12
  float pl_w = out == 7 ? pl : 0.f, vl_w = out == 7 ? vl : 0.f, kl_w = out == 7 ? kl : 0.f;
#pragma unroll
  for (int off = 8; off < 64; off <<= 1) {
    pl_w += __shfl_xor(pl_w, off);
    vl_w += __shfl_xor(vl_w, off);
    kl_w += __shfl_xor(kl_w, off);
  }
  const int wave_ = threadIdx.x >> 6;
  if ((threadIdx.x & 63) < 8) {
    red[wave_ * 20 + 4 + out] = dsum;
    if (out < ACT) red[wave_ * 20 + 12 + out] = gls;
    if (out == 7) {
      red[wave_ * 20 + 0] = pl_w;
      red[wave_ * 20 + 1] = vl_w;
      red[wave_ * 20 + 2] = kl_w;
    }
  }
