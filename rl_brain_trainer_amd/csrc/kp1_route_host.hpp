// kp1_route_host.hpp -- the route handle (include/kp1_route.h) as the translation units of libkp1.so see it: kp1_env.hip owns its entry
// points, kp1_mlp.hip steps it from the route rollout kernel (kp1_mlp_forward_route_step).  Include after kp1_route_step.inc (RouteDevCfg,
// RouteState, RouteTable, RouteChainDev).
#pragma once

#include <vector>

#include "../../include/kp1_route.h"

struct kp1_route {
  kp1_env* base = nullptr;
  int64_t n = 0;               // the base env's env count (kp1_mlp.hip sees kp1_env as an opaque type)
  kp1_route_config cfg;
  int32_t n_waypoints = 0;
  double *q = nullptr, *pose = nullptr, *next_dq = nullptr, *progress = nullptr;  // device
  std::vector<double> h_q, h_pose, h_next, h_progress;
  std::vector<int32_t> h_chunk;
  RouteDevCfg* dev_cfg = nullptr;
  int32_t* ints = nullptr;     // [6][N]
  uint8_t* bytes = nullptr;    // [4][N] flags + [N] base done
  void* reals = nullptr;       // R[2 + 27][N]
  uint64_t* rng64 = nullptr;
  uint32_t* rng32 = nullptr;
  double* scratch = nullptr;   // [N][28]
  double* opt_scratch = nullptr;  // explicit reset options: 3 * [N][7] doubles
  int32_t* opt_ints = nullptr;    // 2 * [N]
  float* base_obs = nullptr;   // [N][56]
  void* base_reward = nullptr; // R[N]
  void* comps = nullptr;       // R[17][N]
  float* fused_actions = nullptr;   // [N][7] clipped actions of kp1_mlp_forward_route_step: what kp1_route_step reads from its caller (f32 handles)
  bool comps_enabled = false;
  int32_t obs_stride = 0;      // row pitch of caller observation buffers (kp1_route_set_obs_stride; default = obs_dim)
  int32_t n_replicas = 1, n_per_replica = 0;   // population handle: K blocks of N envs (a single handle: 1 x N)
  std::vector<int32_t> win;    // host copy of the reset windows [K][2]
  int32_t n_trackers = 0;      // prefix trackers created on this handle and not yet destroyed (a chain refuses a tracked handle)
  int32_t n_chains = 0;        // kp1_route_chain objects created on this handle and not yet destroyed (kp1_mlp_forward_route_step refuses them)
  std::vector<void*> allocs;
};

struct kp1_route_chain {
  RouteChainDev d{};
  int32_t n_rows = 0;
  const kp1_route* owner = nullptr;   // the handle it was created on
  double* init_q = nullptr;    // [R][7] route_q[max(start - 1, 0)]
  int32_t* zeros = nullptr;    // [R] start_route_index = 0
  bool counted = false;        // in kp1_route::n_chains
  std::vector<void*> allocs;
};

namespace {

template <typename R>
RouteState<R> route_state_of(const kp1_route* r) {
  const int64_t n = r->n;
  RouteState<R> s;
  s.cur = r->ints; s.start = r->ints + n; s.last = r->ints + 2 * n; s.streak = r->ints + 3 * n; s.completed = r->ints + 4 * n; s.reset_mode = r->ints + 5 * n;
  s.ready = r->bytes; s.wp_success = r->bytes + n; s.regression = r->bytes + 2 * n; s.ori_hit = r->bytes + 3 * n;
  s.q_error = (R*)r->reals; s.nearest = (R*)r->reals + n; s.prev = (R*)r->reals + 2 * n;
  s.rng64 = r->rng64; s.rng32 = r->rng32; s.scratch = r->scratch;
  s.comps = (r->comps_enabled && r->comps) ? (R*)r->comps : nullptr;
  return s;
}
RouteTable route_table_of(const kp1_route* r) { return RouteTable{r->q, r->pose, r->next_dq, r->progress, r->n_waypoints}; }

}  // namespace
