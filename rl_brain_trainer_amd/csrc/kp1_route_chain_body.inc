// kp1_route_chain_body.inc -- the statements of one chain step of row i (evaluate_sequential_route's host loop between two env steps: the
// per-episode bookkeeping from the planes the route step has just written, and at the end of an episode the waypoint's record and the
// explicit-state hand-over to the next waypoint).  Included as text by the two functions that run it, kp1_route_chain_kernel (kp1_route.inc)
// and route_chain_lane (kp1_route_step.inc), each after its own prologue, which declares
//   a (RouteChainArgs<R>), st (a.st), ch (a.ch), i (the row), alive_after (int, 0).
// One text, so the two functions cannot drift apart; text and not a call from the kernel, because a call form moves the stand-alone
// kernel's register allocation (DESIGN.md sections 22 and 25).
    if (!ch.alive[i]) {
      if (a.tags) { a.tags[2 * i] = -1; a.tags[2 * i + 1] = -1; }
    } else {
      // 1. the step just taken (_roll_one's loop body)
      const int waypoint = ch.wp[i];
      const int steps = ch.steps[i] + 1;
      const float pos = (float)st.r(F_POS_ERR, i), ori = (float)st.r(F_ORI_ERR, i), qerr = (float)a.rs.q_error[i];
      const float min_pos = fminf(ch.min_pos[i], pos), min_ori = fminf(ch.min_ori[i], ori), min_q = fminf(ch.min_q[i], qerr);
      int first_ready = ch.first_ready[i];
      if (a.rs.ready[i] != 0 && first_ready < 0) first_ready = steps;
      const int streak = a.rs.streak[i];
      const int max_streak = ch.max_streak[i] > streak ? ch.max_streak[i] : streak;
      if (a.tags) { a.tags[2 * i] = waypoint; a.tags[2 * i + 1] = steps - 1; }
      const uint8_t d = a.done[i];
      alive_after = 1;
      if (!(d & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED))) {
        ch.steps[i] = steps; ch.first_ready[i] = first_ready; ch.max_streak[i] = max_streak;
        ch.min_pos[i] = min_pos; ch.min_ori[i] = min_ori; ch.min_q[i] = min_q;
      } else {
        // 2. the waypoint's record, then the hand-over
        const bool success = (d & KP1_DONE_SUCCESS) != 0;
        double q0[NJ], dq0[NJ], pa0[NJ];
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
          q0[k] = st.q_load(k, i);
          dq0[k] = (double)st.r(F_DQ + k, i);
          pa0[k] = (double)st.r(F_PREV_ACTION + k, i);
        }
        const int slot = waypoint - ch.start[i];
        if (slot >= 0 && slot < ch.max_len) {
          kp1_route_chain_record& rec = ch.records[i * ch.max_len + slot];
          rec.route_index = waypoint; rec.success = success ? 1 : 0; rec.route_ready_hit = first_ready >= 0 ? 1 : 0;
          rec.max_ready_streak = max_streak; rec.first_ready_step = first_ready; rec.steps = steps;
          rec.final_position_error = (double)pos; rec.final_orientation_error = (double)ori; rec.final_q_error = (double)qerr;
          rec.min_position_error = (double)min_pos; rec.min_orientation_error = (double)min_ori; rec.min_q_error = (double)min_q;
          rec.final_action_magnitude = (double)st.r(F_ACTION_L2, i); rec.final_dq_norm = (double)st.r(F_EXEC_DQ, i);
#pragma unroll
          for (int k = 0; k < NJ; ++k) { rec.final_q[k] = q0[k]; rec.final_dq[k] = dq0[k]; rec.final_prev_action[k] = pa0[k]; }
          ch.n_records[i] = slot + 1;
        }
        if (waypoint >= ch.end[i] || (ch.stop_on_failure && !success)) {
          ch.alive[i] = 0;
          alive_after = 0;
        } else {
          int win_min, win_max;
          route_window_of(*a.rc, i, win_min, win_max);
          route_reset_env<R>(st, *a.cfg, *a.smp, *a.rc, a.rt, a.rs, i, waypoint + 1, 0, KP1_ROUTE_MODE_EXPLICIT, q0, dq0, pa0, a.obs, a.obs_dim,
                             a.obs_stride, win_max);
          route_chain_open<R>(st, ch, i, waypoint + 1);
        }
      }
    }
