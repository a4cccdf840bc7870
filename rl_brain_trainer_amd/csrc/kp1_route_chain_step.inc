// kp1_route_chain_step.inc -- lock steps of the chained route evaluator in ONE launch (kp1_mlp_forward_route_chain_step: one lock step;
// kp1_route_chain_run: n_steps of them) on an Hp = 128 handle: deterministic policy forward of a row tile, the base approach step of the tile's
// envs, the nearest-waypoint scan, the route step without auto-reset, and kp1_route_chain_kernel's per-row statements (accounting, tag, record,
// hand-over to the next waypoint or the end of the row).  Included by kp1_mlp.hip inside its anonymous namespace after
// kp1_route_rollout_step.inc (uses RrGeom, es_layer, head_dot, step_env_lane, store_obs_row, route_nearest_group, route_step_lane,
// route_chain_lane).
//
// Geometry: route_rollout_step_kernel's without the value plane.  grid = (row tiles of ES_BM rows, replicas), 256 threads; row m of replica k is
// env k n + m (rows are replica-major).  One lock step, all ordering by __syncthreads() that all 256 threads reach (rows are masked, never
// exited):
//   forward + clamp (256 threads) | base step (lane r of wave 0 = row r, if its chain is alive) while waves 1-3 bring the route table into LDS
//   | nearest scan (thread t = row t / 8, sub-lane t % 8) | route step (auto_reset 0) and chain step (lane r of wave 0) | the alive rows, as a
//   32-bit mask in one LDS word.
// EPISODE: the workgroup repeats that while its tile has an alive row and the span a.n_steps is not used up.  Nothing crosses a tile (frozen
// policy, no auto-reset, no RNG, every chain array of row i is written by the lane that steps env i), so there is no synchronisation between
// workgroups and the loop is bounded by the span.  The observation row written by the route step (or by the hand-over) is the next x tile:
// the barrier at the bottom of the loop stands between wave 0's stores and the four waves' loads (workgroup scope; the waves share one CU and
// its L1, which the stores write through -- kp1_eval_step.inc's argument).  The route table is converted again in every step: its overlay, the
// x and h1 tiles, is live during the forward.
//
// A row whose chain has ended is NOT stepped (kp1_route_chain_step goes on stepping it; nothing of it is read there): it gets its {-1, -1} tag
// and nothing else of it is written -- env planes, rs.*, its next_obs / action / reward / done entries and the handle's action scratch stay.
// A workgroup whose tile has no alive row at entry writes those tags and leaves.
//
// Bit-identity with kp1_mlp_forward (noise NULL, clipped) + kp1_route_chain_step for every alive row: the forward and the clamp are
// eval_step_kernel's (head_infer_kernel with noise = NULL: act = v); base step, table conversion, scan and route step are
// route_rollout_step_kernel's, phase by phase (x tile and scan as the same included text: kp1_x_tile_body.inc,
// kp1_route_nearest_scan_body.inc), with auto_reset 0 as route_launch_step passes it; the chain step is kp1_route_chain_kernel's text
// (kp1_route_chain_body.inc) on the same inputs read from the same places.  In the EPISODE form the env index, the config address and the
// plane stride carry the loop's run-time zero (es_episode_env's reason: addresses and config reads stay inside the iteration).

struct RouteChainStepArgs {
  RolloutStepArgs fwd;           // fwd.env: the BASE step as route_launch_step launches it (auto_reset 0, outputs = the wrapper's scratch at pitch 56);
                                 // fwd.action: the caller's [K n][7] buffer for the clipped action, or nullptr; noise / value / log_prob unused
  RouteStepArgs<float> route;    // auto_reset 0; route.actions = clipped; route.obs = next_obs (== fwd.obs in place)
  RouteChainDev ch;
  int32_t* tags;                 // [K n][2] or nullptr
  float* clipped;                // [K n][7] the handle's scratch
  int n_steps;                   // EPISODE: lock steps of this launch
};

template <int INP, bool POP, bool EPISODE>
__global__ void __launch_bounds__(ES_NTH) route_chain_step_kernel(const RouteChainStepArgs ra) {
  using G = RrGeom<INP>;
  __shared__ __attribute__((aligned(16))) float lds[G::LDS_FLOATS];
  __shared__ unsigned alive_word;        // the tile's alive rows after the step, bit r = row r
  __shared__ int alive_count;            // and their number
  const RolloutStepArgs& a = ra.fwd;
  float* xs = lds;
  float* h1s = xs + G::X_FLOATS;
  float* h2s = h1s + ES_H_FLOATS;
  float* acts = h2s + ES_H_FLOATS;
  const unsigned rep = blockIdx.y;
  const int m0 = blockIdx.x * ES_BM;
  const int64_t env0 = (int64_t)rep * a.n + m0;          // env of the tile's row 0
  const int rows_live = min(ES_BM, a.n - m0);

  // the tile's alive rows: the same answer in all four waves, nothing has written a flag yet
  unsigned alive_mask;
  {
    const int lane = threadIdx.x & 63;
    alive_mask = (unsigned)__ballot(lane < rows_live && ra.ch.alive[env0 + min(lane, rows_live - 1)] != 0);
    if (!alive_mask) {
      if (ra.tags && threadIdx.x < (unsigned)rows_live) { ra.tags[2 * (env0 + lane)] = -1; ra.tags[2 * (env0 + lane) + 1] = -1; }
      return;
    }
  }
  int step = 0;
  unsigned runtime_zero = 0;             // EPISODE: see es_episode_env

  do {
  // (EPISODE: the thread index carries the loop's run-time zero too, so that what is derived from it -- operand addresses of the layers, the
  // heads and the x tile -- is formed inside the iteration and not held in registers across the env step)
  const int tid = (int)threadIdx.x + (EPISODE ? (int)runtime_zero : 0), lane = tid & 63, wave = tid >> 6;
  const int row = tid >> 3, out = tid & 7;
  // the x-tile load reads what the stepping lanes wrote (in place, and in the previous iteration): no __restrict__ on it
  const float* obs = a.obs + (int64_t)rep * a.n * a.obs_stride;
  const float* __restrict__ w3 = a.w3 + rep * a.r_w3;
  const float* __restrict__ b3 = a.b3 + rep * a.r_b3;
  // ---- 1. the tile's observation rows -> LDS (rows past the replica's last and columns >= Kreal read as zero, as gemm_nt_kernel masks them)
  {
    constexpr int X_INP = INP, X_PITCH = G::XP;
    const int x_n = a.n, x_stride = a.obs_stride, x_kreal = a.Kreal;
#include "kp1_x_tile_body.inc"
  }
  __syncthreads();

  // ---- 2. policy net: h1, h2, the seven heads, the clamp (head_infer_kernel with noise = NULL)
  es_layer<INP>(xs, G::XP, a.w1 + rep * a.r_w1, a.b1 + rep * a.r_b, h1s, wave, lane);
  __syncthreads();
  es_layer<ES_HP>(h1s, ES_HPITCH, a.w2 + rep * a.r_w2, a.b2 + rep * a.r_b, h2s, wave, lane);
  __syncthreads();
  const bool row_alive = ((alive_mask >> row) & 1u) != 0;   // rows past the tile's last are never alive
  {
    float v = 0.f;
    if (out < ACT) {
      v = head_dot(h2s + row * ES_HPITCH, w3 + out * ES_HP, ES_HP) + b3[out];
      v = fminf(fmaxf(v, -1.f), 1.f);
      if (row_alive) {
        const int64_t e = (env0 + row) * ACT + out;
        ra.clipped[e] = v;               // what the route step reads as its caller's action
        if (a.action) a.action[e] = v;
      }
    }
    acts[row * 8 + out] = v;
  }
  __syncthreads();

  // ---- 3. lane r of wave 0 steps base env env0 + r (no auto-reset) if its chain is alive and stores its base observation row to the wrapper's
  //         scratch; meanwhile waves 1-3 convert the route joint table into LDS over the x and h1 tiles (last read two barriers ago)
  const int W = ra.route.rt.n;
  float* route_q = lds;                  // [W][7], W <= KP1_ROUTE_FUSED_MAX_WAYPOINTS (checked by the host)
  const bool lane_alive = wave == 0 && lane < ES_BM && ((alive_mask >> (lane & 31)) & 1u) != 0;
  const int64_t i = env0 + lane + (EPISODE ? runtime_zero : 0u);
  if (wave == 0) {
    if (lane_alive) {
      float o[KP1_OBS_DIM];
      if constexpr (EPISODE) {
        const StepArgs<float> env = es_episode_env(a.env, runtime_zero);
        step_env_lane<float, KP1_MODE_APPROACH, false, POP>(env, i, acts + lane * 8, o);
        store_obs_row(env.obs, i, o, KP1_OBS_DIM);
      } else {
        step_env_lane<float, KP1_MODE_APPROACH, false, POP>(a.env, i, acts + lane * 8, o);
        store_obs_row(a.env.obs, i, o, KP1_OBS_DIM);
      }
    }
  } else {
    const double* __restrict__ tq = ra.route.rt.q;
    for (int e = tid - 64; e < W * NJ; e += ES_NTH - 64) route_q[e] = (float)tq[e];
  }
  __syncthreads();                       // the state planes of the tile's stepped envs are written; the table is in LDS

  // ---- 4. the nearest-waypoint scan: thread t = (row t / 8, sub-lane t % 8)
  {
    const bool scan_store = row_alive;
#include "kp1_route_nearest_scan_body.inc"
  }
  __syncthreads();

  // ---- 5. lane r of wave 0: the route step of env env0 + r without auto-reset (reads the state planes, rs.*, the base done byte and the clipped
  //         action from memory, as kp1_route_step_kernel does), then the chain step of the row; a finished row only gets its tag
  if (wave == 0) {
    int alive_after = 0;
    if (lane < rows_live) {
      RouteChainArgs<float> c;
      if constexpr (EPISODE) {
        RouteStepArgs<float> s = ra.route;
        s.cfg = reinterpret_cast<const DevCfg<float>*>(reinterpret_cast<const char*>(ra.route.cfg) + runtime_zero);
        s.st.n = ra.route.st.n + runtime_zero;
        if (lane_alive) route_step_lane<float>(s, i);
        c.st = s.st; c.cfg = s.cfg;
      } else {
        if (lane_alive) route_step_lane<float>(ra.route, i);
        c.st = ra.route.st; c.cfg = ra.route.cfg;
      }
      c.smp = ra.route.smp; c.rc = ra.route.rc; c.rt = ra.route.rt; c.rs = ra.route.rs; c.ch = ra.ch;
      c.done = ra.route.done; c.obs = ra.route.obs; c.tags = ra.tags; c.obs_dim = ra.route.obs_dim; c.obs_stride = ra.route.obs_stride;
      alive_after = route_chain_lane<float>(c, i);
    }
    const unsigned long long bal = __ballot(alive_after != 0);
    if (lane == 0) { alive_word = (unsigned)bal; alive_count = __popcll(bal); }
  }
  __syncthreads();                       // the tile's new observation rows and the alive rows, for all four waves
  alive_mask = __builtin_amdgcn_readfirstlane(alive_word);
  if constexpr (EPISODE) runtime_zero = (unsigned)__builtin_amdgcn_readfirstlane(alive_count) >> 31;   // a count is never negative
  } while (EPISODE && alive_mask != 0 && ++step < ra.n_steps);
  if (threadIdx.x == 0 && alive_mask) atomicAdd(ra.ch.n_alive, __popc(alive_mask));
}
