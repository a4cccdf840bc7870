// kp1_route_rollout_step.inc -- one rollout step of a ROUTE env in ONE launch (kp1_mlp_forward_route_step on an Hp = 128 handle): stochastic
// policy forward of a row tile (both nets), Gaussian sampling, the base approach step of the tile's envs, the nearest-waypoint scan and the
// route step with its wrapper-level auto-reset.  Included by kp1_mlp.hip inside its anonymous namespace after kp1_mlp_fused.inc and
// kp1_route_step.inc (uses es_layer and the ES_* geometry, head_dot, step_env_lane, store_obs_row, route_nearest_group, route_step_lane).
//
// Hidden 64 / 128 in the Hp = 128 layout.  INP = 64: the 56-float route observation (include_route_keys off) at pitch 56 or 64; INP = 128: the
// 80-float observation at pitch 80 or 128.  grid = (row tiles of ES_BM rows, replicas, value ? 2 : 1), 256 threads; row m of replica k is env
// k n + m of the route handle.  Plane z = 1 is rollout_step_kernel's value plane.  Plane z = 0, all ordering by __syncthreads():
//   forward + sampling (256 threads) | base step (lane r of wave 0 = row r) while waves 1-3 bring the route table into LDS | nearest scan
//   (thread t = row t / 8, sub-lane t % 8: 32 rows x 8 lanes is the workgroup) | route step with auto-reset (lane r of wave 0).
// Every barrier is reached by all 256 threads: dead rows are masked, never exited.
//
// Bit-identity with launch_forward_layers + head_infer_kernel + kp1_step_kernel + kp1_route_nearest_kernel + kp1_route_step_kernel:
//  * forward, heads, sampling tail: the argument at the top of kp1_rollout_step.inc, and for the x tile and the tail its very text
//    (kp1_x_tile_body.inc, kp1_sample_tail_body.inc; the scan below is kp1_route_nearest_scan_body.inc, shared with the chain kernel); layer 1 at INP = 128 is es_layer<128>, the chain layer 2
//    issues at either width (all k groups, the zero columns past the observation width included, as gemm_nt_kernel issues them).
//  * base step: step_env_lane is the body of kp1_step_kernel; as there, its observation row is stored (to the wrapper's scratch, which nothing
//    reads; row by row, which leaves LDS to the table) so that the same values stay live in both kernels, and its done byte goes to the
//    wrapper's scratch byte, which the route step reads.
//  * nearest scan: the table is converted with kp1_route_nearest_kernel's expression (float)rt.q[e], q is read from the state planes the stepping
//    lane has just written (a barrier in between), rows past the replica's last clamp to the last live row as that kernel clamps, and
//    route_nearest_group is that kernel's loop and shuffles.
//  * route step: route_step_lane is the body of kp1_route_step_kernel and reads every input where that kernel reads it: the state planes,
//    rs.*, the base done byte, and the clipped action from global memory (the handle's [N][7] scratch, written by the sampling tail with the
//    value kp1_mlp_forward stores as `clipped_action`).  Nothing is handed over in registers.
// No float atomics; every output element has one writer.

constexpr int RR_MAX_INP = 128;
template <int INP>
struct RrGeom {
  static constexpr int XP = INP + 4;                           // LDS pitch of the x tile (K + 4, as ES_XP)
  static constexpr int X_FLOATS = ES_BM * XP;
  static constexpr int OVERLAY_FLOATS = X_FLOATS + ES_H_FLOATS;   // x and h1 tiles: dead after layer 2
  static constexpr int LDS_FLOATS = X_FLOATS + 2 * ES_H_FLOATS + ES_BM * 8;
};
static_assert(RrGeom<ES_INP>::X_FLOATS == ES_X_FLOATS, "INP = 64 is rollout_step_kernel's geometry");
static_assert(RrGeom<ES_INP>::OVERLAY_FLOATS / NJ == KP1_ROUTE_FUSED_MAX_WAYPOINTS,
              "KP1_ROUTE_FUSED_MAX_WAYPOINTS (kp1_route.h) = the waypoints whose joint table fits the smaller overlay, the x + h1 tiles of INP = 64");
static_assert(sizeof(float) * RrGeom<RR_MAX_INP>::LDS_FLOATS <= 64 * 1024, "static LDS");

struct RouteRolloutStepArgs {
  RolloutStepArgs fwd;           // fwd.env: the BASE step as route_launch_step launches it (auto_reset 0, no terminal observation, outputs = the
                                 // wrapper's scratch at pitch 56); the forward's fields as in rollout_step_kernel
  RouteStepArgs<float> route;    // auto_reset 1; route.actions = clipped; route.obs = next_obs
  float* clipped;                // [K n][7] the handle's scratch
};

template <int INP, bool POP>
__global__ void __launch_bounds__(ES_NTH) route_rollout_step_kernel(const RouteRolloutStepArgs ra) {
  using G = RrGeom<INP>;
  __shared__ __attribute__((aligned(16))) float lds[G::LDS_FLOATS];
  const RolloutStepArgs& a = ra.fwd;
  float* xs = lds;
  float* h1s = xs + G::X_FLOATS;
  float* h2s = h1s + ES_H_FLOATS;
  float* acts = h2s + ES_H_FLOATS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned rep = blockIdx.y, net = blockIdx.z;
  const int m0 = blockIdx.x * ES_BM;
  const int64_t env0 = (int64_t)rep * a.n + m0;          // env of the tile's row 0

  // ---- 1. the tile's observation rows -> LDS (rows past the replica's last and columns >= Kreal read as zero, as gemm_nt_kernel masks them)
  {
    constexpr int X_INP = INP, X_PITCH = G::XP;
    const int x_n = a.n, x_stride = a.obs_stride, x_kreal = a.Kreal;
    const float* __restrict__ obs = a.obs + (int64_t)rep * a.n * a.obs_stride;
#include "kp1_x_tile_body.inc"
  }
  __syncthreads();

  // ---- 2. hidden layers of this plane's net
  es_layer<INP>(xs, G::XP, a.w1 + rep * a.r_w1 + net * a.n_w1, a.b1 + rep * a.r_b + net * a.n_b, h1s, wave, lane);
  __syncthreads();
  es_layer<ES_HP>(h1s, ES_HPITCH, a.w2 + rep * a.r_w2 + net * a.n_w2, a.b2 + rep * a.r_b + net * a.n_b, h2s, wave, lane);
  __syncthreads();

  const int row = tid >> 3, out = tid & 7;
  const bool ok = m0 + row < a.n;
  const float* __restrict__ w3 = a.w3 + rep * a.r_w3;
  const float* __restrict__ b3 = a.b3 + rep * a.r_b3;

  // ---- z = 1: the value head of the tile's rows (a workgroup of its own: it meets none of the barriers below)
  if (net != 0) {
    if (ok && out == HEADS - 1) a.value[env0 + row] = head_dot(h2s + row * ES_HPITCH, w3 + out * ES_HP, ES_HP) + b3[out];
    return;
  }

  // ---- 3. z = 0: action heads and head_infer_kernel's sampling tail
  {
    constexpr bool TAIL_STORES_CLIPPED = true;   // what the route step reads as its caller's action
    const RolloutStepArgs& fw = a;
    const int64_t tail_off = 0;
    float* const tail_clipped = ra.clipped;
#include "kp1_sample_tail_body.inc"
  }
  __syncthreads();

  // ---- 4. lane r of wave 0 steps base env env0 + r (no auto-reset) and stores its base observation row to the wrapper's scratch; meanwhile
  //         waves 1-3 convert the route joint table into LDS over the x and h1 tiles (last read two barriers ago)
  const int rows_live = min(ES_BM, a.n - m0);
  const int W = ra.route.rt.n;
  float* route_q = lds;                  // [W][7], W <= KP1_ROUTE_FUSED_MAX_WAYPOINTS (checked by the host)
  if (wave == 0) {
    if (lane < rows_live) {
      float o[KP1_OBS_DIM];
      step_env_lane<float, KP1_MODE_APPROACH, false, POP>(a.env, env0 + lane, acts + lane * 8, o);
      store_obs_row(a.env.obs, env0 + lane, o, KP1_OBS_DIM);
    }
  } else {
    const double* __restrict__ tq = ra.route.rt.q;
    for (int e = tid - 64; e < W * NJ; e += ES_NTH - 64) route_q[e] = (float)tq[e];
  }
  __syncthreads();                       // the state planes of the tile's envs are written; the table is in LDS

  // ---- 5. the nearest-waypoint scan: thread t = (row t / 8, sub-lane t % 8)
  {
    const bool scan_store = ok;
#include "kp1_route_nearest_scan_body.inc"
  }
  __syncthreads();

  // ---- 6. lane r of wave 0: the route step of env env0 + r, wrapper-level auto-reset included (reads the state planes, rs.* and the base done
  //         byte from memory, as kp1_route_step_kernel does)
  if (wave == 0 && lane < rows_live) route_step_lane<float>(ra.route, env0 + lane);
}
