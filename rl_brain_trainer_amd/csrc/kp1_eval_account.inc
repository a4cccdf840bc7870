// kp1_eval_account.inc -- the evaluator's per-episode bookkeeping of one env step (step >= 1 of kp1_eval_accumulate).
// Included inside an anonymous namespace by kp1_env.hip (eval_accumulate_kernel: one lane per episode after a kp1_step launch) and by
// kp1_mlp.hip (eval_step_kernel, kp1_eval_step.inc: the lane that has just stepped the env does the bookkeeping in the same launch), so both
// execute the same expressions.  Needs kp1_device.hpp (the F_* field indices) and kp1.h (kp1_eval_buffers, KP1_DONE_*).

// STATE_W = the 34 leading real fields of the handle (q, dq, prev_action, goal_q, goal_pose6: F_Q .. F_GOAL_POSE + 5).
constexpr int EVAL_STATE_W = F_GOAL_POSE + 6;
static_assert(EVAL_STATE_W == 34 && F_Q == 0, "kp1_eval_buffers::state is the leading 34 fields of the handle");

// Episode i (env i of the handle whose real planes are `real`, n envs) after env step number `step` (>= 1): `an` = norm of the action applied,
// `d` = the step's done byte.  Returns 1 when the episode is still alive after this step, 0 when it has finished (or had finished before).
// `real` carries no __restrict__: eval_step_kernel reads here what step_env_lane stored a few instructions earlier in the same lane.
template <typename R>
__device__ __forceinline__ int eval_account_step(const R* real, int n, int i, const kp1_eval_buffers& b, double an, uint8_t d, int step, bool track_ready,
                                                 double thr_pos, double thr_ori, double thr_act, double thr_dq, int confirm) {
  double* M = b.metrics;
  int32_t* C = b.counters;
  uint8_t* F = b.flags;
  if (!F[i]) return 0;
  const double pos = (double)real[(size_t)F_POS_ERR * n + i], ori = (double)real[(size_t)F_ORI_ERR * n + i];
  const double dqn = (double)real[(size_t)F_EXEC_DQ * n + i];
  const uint8_t succ = (d & KP1_DONE_SUCCESS) ? 1 : 0;
  C[i] = step;
  M[6 * (size_t)n + i] += an;
  M[7 * (size_t)n + i] += dqn;
  M[0 * (size_t)n + i] = pos; M[1 * (size_t)n + i] = ori; M[4 * (size_t)n + i] = an; M[5 * (size_t)n + i] = dqn;
  const double mp = fmin(M[2 * (size_t)n + i], pos), mo = fmin(M[3 * (size_t)n + i], ori);
  M[2 * (size_t)n + i] = mp; M[3 * (size_t)n + i] = mo;
  F[1 * (size_t)n + i] = succ;
  double st[EVAL_STATE_W];
  for (int f = 0; f < EVAL_STATE_W; ++f) {
    st[f] = (double)real[(size_t)f * n + i];
    b.state[(size_t)i * EVAL_STATE_W + f] = st[f];
  }
  if (track_ready) {
    bool rdy = thr_pos > 0.0 && thr_ori > 0.0 && pos <= thr_pos && ori <= thr_ori;
    if (thr_act > 0.0) rdy = rdy && an <= thr_act;
    if (thr_dq > 0.0) rdy = rdy && dqn <= thr_dq;
    if (rdy) {
      F[2 * (size_t)n + i] = 1;
      if (C[2 * (size_t)n + i] < 0) C[2 * (size_t)n + i] = step;
    }
    const int streak = rdy ? C[3 * (size_t)n + i] + 1 : 0;
    C[3 * (size_t)n + i] = streak;
    if (streak > C[1 * (size_t)n + i]) C[1 * (size_t)n + i] = streak;
    // first-confirmed handoff snapshot.  `ready_streak >= handoff_confirm_steps` as the reference writes it (eval_pipeline_ablation.py:103):
    // with confirm <= 0 it holds at step 1 whatever the streak.  Whether a snapshot is wanted at all is "hand_metrics given".
    if (b.hand_metrics && !F[3 * (size_t)n + i] && streak >= confirm) {
      F[3 * (size_t)n + i] = 1;
      double* H = b.hand_metrics;
      H[0 * (size_t)n + i] = pos; H[1 * (size_t)n + i] = ori; H[2 * (size_t)n + i] = an; H[3 * (size_t)n + i] = dqn;
      H[4 * (size_t)n + i] = mp; H[5 * (size_t)n + i] = mo;
      H[6 * (size_t)n + i] = M[6 * (size_t)n + i]; H[7 * (size_t)n + i] = M[7 * (size_t)n + i];   // sums up to and including this step (:111-112)
      b.hand_step[i] = step;
      b.hand_success[i] = succ;
      for (int f = 0; f < EVAL_STATE_W; ++f) b.hand_state[(size_t)i * EVAL_STATE_W + f] = st[f];
    }
  }
  const uint8_t still = (d & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) ? 0 : 1;
  F[i] = still;
  return still;
}
