// kp1_host.hpp -- host-side helpers shared by the translation units of libkp1.so.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>

#include "../../include/kp1.h"

struct kp1_route;

namespace kp1 {
inline thread_local std::string g_last_error;
inline int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

// hipError_t -> kp1_status: the caller can tell "no GPU" from "out of memory" from "launch rejected" from "an earlier kernel faulted"
inline int status_of(hipError_t e) {
  switch (e) {
    case hipErrorNoDevice:
    case hipErrorInvalidDevice:
    case hipErrorInsufficientDriver:
      return KP1_ERR_NO_DEVICE;
    case hipErrorOutOfMemory:
      return KP1_ERR_ALLOC;
    case hipErrorInvalidConfiguration:
    case hipErrorLaunchOutOfResources:
    case hipErrorInvalidDeviceFunction:
    case hipErrorSharedObjectInitFailed:
      return KP1_ERR_LAUNCH;
    default:
      return KP1_ERR_RUNTIME;
  }
}
// Launch check.  Kernel launches are asynchronous: hipGetLastError() only reports a launch the runtime refused, a fault inside the
// kernel surfaces at a later, unrelated call (as KP1_ERR_RUNTIME).  KP1_SYNC_CHECK=1 in the environment makes every entry point wait
// for its own kernels and report their faults itself (debugging aid: serialises the stream, cannot be used under hipGraph capture).
inline bool sync_check_enabled() {
  static const bool on = [] { const char* e = std::getenv("KP1_SYNC_CHECK"); return e && e[0] && e[0] != '0'; }();
  return on;
}
inline hipError_t launch_status() {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && sync_check_enabled()) e = hipDeviceSynchronize();
  return e;
}
// kp1_env.hip -> kp1_mlp.hip: the kernel-argument block of one fp32 env step (StepArgs<float> of kp1_env_step.inc, copied into `out`), for the
// rollout kernel that runs the policy forward and the env step in one launch.  Fails for fp64 handles and while reward components are on.
int env_step_args_f32(kp1_env* env, void* out, size_t out_bytes, const void* actions, float* obs, void* reward, uint8_t* done, float* terminal_obs,
                      int auto_reset, int* mode, int64_t* n_envs, int* device);
// The same block for the rollout kernel of the layer-wise widths (rollout_step_kernel), which also steps population env handles: accepts a
// handle with bound population stages or dock stage records, reports its replica count (0: unbound) and whether kp1_step would launch the
// population form of the step kernel on it (pop_form).  Fails as above, and for a bound handle whose mode kp1_step refuses.
int env_step_args_f32_population(kp1_env* env, void* out, size_t out_bytes, float* obs, void* reward, uint8_t* done, float* terminal_obs,
                                 int auto_reset, int* mode, int64_t* n_envs, int* device, int* pop_replicas, int* pop_form);
// what the handle's auto-resets follow: the device stage word of kp1_bind_stage_ptr and the tracker array of kp1_bind_population_stages (either
// may be nullptr), whether or not the config has curriculum stages.  kp1_rollout_run checks them against the trackers it is asked to drive.
void env_bound_stage_source(const kp1_env* env, const void** stage_ptr, const void** pop_states);
// kp1_env.hip -> kp1_mlp.hip: what a route chain cannot run on (an fp64 base env, route.sequence, recorded reward components, an attached prefix
// tracker); text for kp1_last_error, or nullptr
const char* route_chain_refusal(const kp1_route* r);
// kp1_mlp_line.hip <- kp1_mlp.hip: the launches only a handle with a hyper-parameter line makes (kp1_mlp_hparams_store).  Their kernels live in
// a code object of their own; the argument blocks (FusedArgs of kp1_mlp_tile.inc, HeadArgs of kp1_mlp.hip: the same text in both units) travel
// as bytes, as StepArgs does above.  start / stop: the profile events of the launch, or nullptr.
int mlp_line_launch_tile(const void* fused_args, size_t bytes, const float* line, dim3 grid, hipEvent_t start, hipEvent_t stop, hipStream_t stream);
int mlp_line_launch_head_train256(const void* head_args, size_t bytes, dim3 grid, size_t lds_bytes, hipStream_t stream);
// table[0 .. n_floats) = v[0 .. n_floats), the values as kernel arguments of one launch; n_floats <= KP1_MLP_MAX_REPLICAS entries
int mlp_line_store(float* table, const float* v, int n_floats, hipStream_t stream);
}  // namespace kp1

#define HIP_TRY(expr)                                                                                              \
  do {                                                                                                             \
    hipError_t _e = (expr);                                                                                        \
    if (_e != hipSuccess) return kp1::fail(kp1::status_of(_e), std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

namespace kp1 {
// the device of an entry point that takes a device index (the stateless ones, and the creators of handles): refused when out of range, else current
inline int use_device(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(KP1_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
  if (device < 0 || device >= count) return fail(KP1_ERR_INVALID, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  return KP1_OK;
}
}  // namespace kp1
