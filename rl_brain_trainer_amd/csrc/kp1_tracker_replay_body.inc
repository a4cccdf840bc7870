// kp1_tracker_replay_body.inc -- the serial PointCurriculum replay of the finished episodes one lane saw, in env order (bit b of m = env b of
// the lane's block, sm = its success bit): count; ring append while the window fills, else overwrite of the oldest entry; window sum; no
// promotion at the last stage, before min_episodes or before the window is full; the rate and its test in double; the event record; the reset
// of count and window.  Included as text by curriculum_scan (kp1_ppo.hip: the ring in LDS, the limits read through c.) and by the TRACK form
// of rollout_run_kernel (kp1_rollout_run.inc: the ring in the tracker, the limits in locals), each after its own prologue, which declares
//   m (unsigned long long, consumed), sm (const unsigned long long), ring (int*, or a reference to the int array),
//   stage, count, len, head, sum, n_events (int, updated), window, max_stage, min_episodes (int), threshold (double), timesteps (long long),
//   st (kp1_curriculum_state*: its events[] are written) and TRK_STORES_STAGE (constexpr bool: st->stage_index is stored at a promotion,
//   for the env steps that follow in the same launch).
// One text, so the two trackers cannot drift; text and not a call, see DESIGN section 28.
  while (m) {
    const int b = __ffsll((long long)m) - 1;
    m &= m - 1;
    const int success = (int)((sm >> b) & 1ull);
    count += 1;
    if (len < window) {
      ring[head + len < window ? head + len : head + len - window] = success;
      len += 1;
      sum += success;
    } else {
      sum += success - ring[head];
      ring[head] = success;
      head = head + 1 < window ? head + 1 : 0;
    }
    if (stage >= max_stage) continue;
    if (count < min_episodes) continue;
    if (len < window) continue;
    const double rate = (double)sum / (double)len;
    if (rate >= threshold) {
      if (n_events < KP1_CURRICULUM_MAX_HISTORY) {
        kp1_curriculum_event& ev = st->events[n_events];
        ev.total_timesteps = timesteps;
        ev.from_stage = stage;
        ev.to_stage = stage + 1;
        ev.trigger_success_rate = rate;
      }
      n_events += 1;
      stage += 1;
      count = 0;
      len = 0;
      head = 0;
      sum = 0;
      if constexpr (TRK_STORES_STAGE) st->stage_index = stage;
    }
  }
