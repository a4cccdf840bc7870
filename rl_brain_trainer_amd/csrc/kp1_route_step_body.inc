// kp1_route_step_body.inc -- the statements of one route step of env i (route_env.py:124-192 / route_sequence_env.py:150-236), after the base
// step has advanced the base env and rs.nearest[i] is written.  Included as text by the two functions that run it, kp1_route_step_kernel
// (kp1_route.inc) and route_step_lane (kp1_route_step.inc), each after its own prologue, which declares
//   a (RouteStepArgs<R>), route_q (a.rt.q), W (a.rt.n), i (the env), n (a.st.n).
// One text, so the two functions cannot drift apart; text and not a call from the kernel, because the call form changed the stand-alone
// kernel's register allocation (DESIGN.md section 22).
  const DevCfg<R>& cfg = *a.cfg;
  const RouteDevCfg& rc = *a.rc;
  const kp1_route_reward& w = rc.c.reward;
  const EnvState<R>& st = a.st;
  const RouteState<R>& rs = a.rs;
  const R Z = (R)0;

  R prev_q[NJ], prev_dq[NJ], prev_action[NJ], prev_pose[6], act[NJ], q[NJ], dq[NJ], pose[6];
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    prev_q[k] = rs.prev[(RP_Q + k) * n + i];
    prev_dq[k] = rs.prev[(RP_DQ + k) * n + i];
    prev_action[k] = rs.prev[(RP_ACT + k) * n + i];
    act[k] = a.actions[i * NJ + k];          // the wrappers use the raw action (np.asarray(action)), not the base env's clipped copy
    q[k] = st.r(F_Q + k, i);
    dq[k] = st.r(F_DQ + k, i);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    prev_pose[k] = rs.prev[(RP_POSE + k) * n + i];
    pose[k] = st.r(F_EE_POSE + k, i);
  }
  const int target = rs.cur[i];
  const int wt = rclipi(target, 0, W - 1), wtan = rclipi(target - 1 > 0 ? target - 1 : 0, 0, W - 1);
  R goal_q[NJ], goal_pose[6], tangent[NJ];
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    goal_q[k] = (R)route_q[wt * NJ + k];
    tangent[k] = (R)a.rt.next_dq[wtan * NJ + k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) goal_pose[k] = (R)a.rt.pose[wt * 6 + k];

  R d[NJ];
#pragma unroll
  for (int k = 0; k < NJ; ++k) d[k] = goal_q[k] - q[k];
  const R curr_q_err = norm7<R>(d);
#pragma unroll
  for (int k = 0; k < NJ; ++k) d[k] = goal_q[k] - prev_q[k];
  const R prev_q_err = norm7<R>(d);
  const R action_norm = norm7<R>(act), dq_norm = norm7<R>(dq), tangent_norm = norm7<R>(tangent);
  const R nearest = rs.nearest[i];   // kp1_route_nearest_kernel, launched between the base step and this kernel
  const R base_pos = st.r(F_POS_ERR, i), base_ori = st.r(F_ORI_ERR, i);  // info["position_error_norm"] etc. of the base step
  const bool ready = curr_q_err <= (R)w.route_ready_q_threshold && base_pos <= (R)w.route_ready_pos_threshold_m &&
                     base_ori <= (R)w.route_ready_ori_threshold_rad && action_norm <= (R)w.route_ready_action_threshold &&
                     dq_norm <= (R)w.route_ready_dq_threshold;
  int streak = ready ? rs.streak[i] + 1 : 0;

  // compute_route_reward (reward_route.py:54-143)
  R pe[3], oe[3], prev_pos, prev_ori, curr_pos, curr_ori;
  pose_error_norms<R>(prev_pose, goal_pose, pe, oe, &prev_pos, &prev_ori);
  pose_error_norms<R>(pose, goal_pose, pe, oe, &curr_pos, &curr_ori);
  R dot = Z;
#pragma unroll
  for (int k = 0; k < NJ; ++k) dot += (q[k] - prev_q[k]) * tangent[k];
  const R tangent_progress = tangent_norm > Z ? dot / kp_max<R>(tangent_norm, (R)1e-9) : Z;
  const bool ready_r = curr_q_err <= (R)w.route_ready_q_threshold && curr_pos <= (R)w.route_ready_pos_threshold_m &&
                       curr_ori <= (R)w.route_ready_ori_threshold_rad && action_norm <= (R)w.route_ready_action_threshold &&
                       dq_norm <= (R)w.route_ready_dq_threshold;
  R low_motion = Z;
  if (curr_pos <= (R)2 * (R)w.route_ready_pos_threshold_m && curr_ori <= (R)2 * (R)w.route_ready_ori_threshold_rad) {
    const R action_clean = kp_max<R>((R)1 - action_norm / kp_max<R>((R)w.route_ready_action_threshold, (R)1e-9), Z);
    const R dq_clean = kp_max<R>((R)1 - dq_norm / kp_max<R>((R)w.route_ready_dq_threshold, (R)1e-9), Z);
    low_motion = (R)w.low_motion_near_waypoint_bonus * (R)0.5 * (action_clean + dq_clean);
  }
  R a2 = Z, da2 = Z;
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    a2 += act[k] * act[k];
    const R t = act[k] - prev_action[k];
    da2 += t * t;
  }
  R comps[KP1_ROUTE_N_COMPONENTS];
  comps[0] = (R)w.q_goal_progress_weight * (prev_q_err - curr_q_err);
  comps[1] = (R)w.ee_position_progress_weight * (prev_pos - curr_pos);
  comps[2] = (R)w.ee_orientation_progress_weight * (prev_ori - curr_ori);
  comps[3] = (R)w.route_tangent_progress_weight * kp_max<R>(tangent_progress, Z);
  comps[4] = ready_r ? (R)w.same_step_route_ready_bonus : Z;
  comps[5] = (ready_r && streak >= 1) ? (R)w.route_ready_dwell_bonus : Z;
  comps[6] = low_motion;
  comps[7] = -(R)w.orientation_regression_penalty_weight * kp_max<R>(curr_ori - prev_ori, Z);
  comps[8] = -(R)w.q_route_regression_penalty_weight * kp_max<R>(curr_q_err - prev_q_err, Z);
  comps[9] = -(R)w.off_route_penalty_weight * kp_max<R>(nearest, Z);
  comps[10] = -(R)w.action_magnitude_weight * (a2 / (R)7) + -(R)w.action_delta_weight * (da2 / (R)7);
  comps[11] = -(R)w.dq_penalty_weight * dq_norm;
  comps[12] = (curr_q_err >= prev_q_err && curr_pos >= prev_pos && curr_ori >= prev_ori) ? -(R)w.no_progress_penalty : Z;
  comps[13] = curr_q_err; comps[14] = curr_pos; comps[15] = curr_ori; comps[16] = ready_r ? (R)1 : Z;
  R reward = Z;
#pragma unroll
  for (int k = 0; k < 13; ++k) reward += comps[k];
  if (rs.comps) {
#pragma unroll
    for (int k = 0; k < KP1_ROUTE_N_COMPONENTS; ++k) rs.comps[(int64_t)k * n + i] = comps[k];
  }

  const uint8_t bd = a.base_done[i];
  const bool base_terminated = (bd & KP1_DONE_TERMINATED) != 0, truncated = (bd & KP1_DONE_TRUNCATED) != 0;
  const bool base_success = (bd & KP1_DONE_SUCCESS) != 0 && (bd & KP1_DONE_INVALID) == 0;
  const bool reached = ready && streak >= rc.success_dwell_steps;
  bool terminated = false, success = false, retarget = false;
  int cur = target, completed = rs.completed[i];
  if (rc.c.sequence_enabled) {
    if (reached) {
      completed += 1;
      if (target >= rs.last[i]) {
        success = true;
        terminated = true;
      } else {
        cur = target + 1;  // _advance_target (route_sequence_env.py:253-257)
        retarget = true;
        if (rc.c.reset_ready_streak_on_advance) streak = 0;
      }
    }
    if (base_terminated && !terminated && !base_success) terminated = true;
  } else {
    success = reached;
    terminated = base_terminated;
    if (base_terminated && base_success && !success) terminated = false;
    if (success && rc.terminate_on_success) terminated = true;
  }

  float o[KP1_OBS_DIM];
  R pa_now[NJ];
#pragma unroll
  for (int k = 0; k < NJ; ++k) pa_now[k] = st.r(F_PREV_ACTION + k, i);
  if (retarget) {
    const int wn = rclipi(cur, 0, W - 1);
    R ng[6];
#pragma unroll
    for (int k = 0; k < NJ; ++k) st.r(F_GOAL_Q + k, i) = (R)route_q[wn * NJ + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      ng[k] = (R)a.rt.pose[wn * 6 + k];
      st.r(F_GOAL_POSE + k, i) = ng[k];
    }
    R pn, on;
    pose_error_norms<R>(pose, ng, pe, oe, &pn, &on);
    st.r(F_ENTRY + 0, i) = pn;          // _capture_entry_metrics (arm_kinematic_env.py:425-430)
    st.r(F_ENTRY + 1, i) = on;
    st.r(F_ENTRY + 2, i) = norm7<R>(pa_now);
    st.r(F_ENTRY + 3, i) = norm7<R>(dq);
  } else {
    R cg[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) cg[k] = st.r(F_GOAL_POSE + k, i);
    R pn, on;
    pose_error_norms<R>(pose, cg, pe, oe, &pn, &on);
  }
  build_observation<R>(cfg, KP1_MODE_APPROACH, q, dq, pa_now, pe, oe, st.iv(I_STEP, i), st.iv(I_DWELL, i), o);

  rs.ready[i] = ready; rs.wp_success[i] = reached; rs.regression[i] = curr_q_err > prev_q_err;
  rs.ori_hit[i] = base_ori <= (R)w.route_ready_ori_threshold_rad;
  rs.q_error[i] = curr_q_err; rs.nearest[i] = nearest;
  rs.cur[i] = cur; rs.streak[i] = streak; rs.completed[i] = completed;
  a.reward[i] = reward;
  a.done[i] = (uint8_t)((terminated ? KP1_DONE_TERMINATED : 0) | (truncated ? KP1_DONE_TRUNCATED : 0) | (success ? KP1_DONE_SUCCESS : 0) |
                        ((bd & KP1_DONE_INVALID) ? KP1_DONE_INVALID : 0));
  if ((terminated || truncated) && a.auto_reset) {
    if (a.terminal_obs) store_route_obs<R>(a.terminal_obs, i, a.obs_dim, a.obs_stride, o, cfg, a.rt, cur, q);
    Pcg g;
    rng_load(rs.rng64, rs.rng32, n, i, g);
    int win_min, win_max;
    route_window_of(rc, i, win_min, win_max);
    RouteSampleDev s;
    sample_route_reset_dev(g, a.rt, *a.smp, rc.c.reset, win_min, win_max, s);
    rng_store(rs.rng64, rs.rng32, n, i, g);
    route_reset_env<R>(st, cfg, *a.smp, rc, a.rt, rs, i, s.route_index, s.start_index, s.mode, s.initial_q, s.initial_dq, s.initial_prev_action, a.obs,
                       a.obs_dim, a.obs_stride, win_max);
    // the finished episode's info stays readable, like the base env's auto-reset
    rs.cur[i] = rs.cur[i];
  } else {
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
      rs.prev[(RP_Q + k) * n + i] = q[k];
      rs.prev[(RP_DQ + k) * n + i] = dq[k];
      rs.prev[(RP_ACT + k) * n + i] = pa_now[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) rs.prev[(RP_POSE + k) * n + i] = pose[k];
    store_route_obs<R>(a.obs, i, a.obs_dim, a.obs_stride, o, cfg, a.rt, cur, q);
  }
