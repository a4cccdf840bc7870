// kp1_route_nearest_scan_body.inc -- the nearest-waypoint scan of a row tile, thread t = (row t / 8, sub-lane t % 8): q is read from the state
// planes the stepping lane has just written (a barrier in between), rows past the replica's last clamp to the last live row as
// kp1_route_nearest_kernel clamps (whole groups of 8 lanes stay in the shuffles), and route_nearest_group is that kernel's loop and shuffles.
// Included as text by route_rollout_step_kernel and route_chain_step_kernel, each inside a braced block after its own prologue, which declares
//   scan_store (const bool: the row's distance is stored -- the row exists / its chain is alive),
//   ra (the kernel's arguments: ra.route), route_q (float*, the table in LDS), W, row, out, rows_live (int), env0 (int64_t).
// One text, so the copies cannot drift; text and not a call, see DESIGN section 28.
  const int64_t ic = env0 + min(row, rows_live - 1);
  float q[NJ];
#pragma unroll
  for (int k = 0; k < NJ; ++k) q[k] = ra.route.st.r(F_Q + k, ic);
  const float d = route_nearest_group<float>(route_q, W, out, q);
  if (out == 0 && scan_store) ra.route.rs.nearest[env0 + row] = d;
