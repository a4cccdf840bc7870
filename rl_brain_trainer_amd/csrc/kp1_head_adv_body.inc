// kp1_head_adv_body.inc -- the advantage normalisation constants of a minibatch, left in adv_ms[0] (mean) and adv_ms[1] (1 / std) by thread 0:
// mode 1 sums the per-block fp64 partials of adv_partials_kernel in a fixed order (wave 0; a.n_adv_partials <= 128) and forms torch's
// .mean() / .std() (unbiased); mode 2 reads them from a.adv_stats, mode 3 from the scalars, mode 0 leaves (0, 1).
// Included as text by head_train_kernel and train_tile128_kernel, each after its own prologue, which declares
//   a (const HeadArgs, the replica's), adv_ms (float*, LDS);
// the site's next barrier publishes adv_ms.  One text, so the copies cannot drift; text and not a call, see DESIGN section 28.
  double ps = 0.0, pss = 0.0;
  if (a.adv_mode == 1 && threadIdx.x < 64) {
    for (int k = threadIdx.x; k < a.n_adv_partials; k += 64) {
      ps += a.adv_partials[2 * k];
      pss += a.adv_partials[2 * k + 1];
    }
    for (int off = 32; off > 0; off >>= 1) {
      ps += __shfl_xor(ps, off);
      pss += __shfl_xor(pss, off);
    }
  }
  if (threadIdx.x == 0) {
    float mean = 0.f, inv_std = 1.f;
    if (a.adv_mode == 1) {  // statistics of this minibatch, torch .mean() / .std() (unbiased)
      const double s = ps, ss = pss;
      const double m = s / a.n;
      const double var = a.n > 1 ? fmax((ss - a.n * m * m) / (a.n - 1), 0.0) : 0.0;
      mean = (float)m;
      inv_std = (float)(1.0 / (sqrt(var) + 1e-8));
    } else if (a.adv_mode == 2) {
      mean = a.adv_stats[0];
      inv_std = a.adv_stats[1];
    } else if (a.adv_mode == 3) {
      mean = a.adv_mean;
      inv_std = a.adv_inv_std;
    }
    adv_ms[0] = mean;
    adv_ms[1] = inv_std;
  }
