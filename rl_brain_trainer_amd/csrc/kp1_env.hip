// kp1_env.hip -- kernels + C ABI (include/kp1.h) of the MI355X kinematic_phase1 rollout engine.
//
// Kernels (all: one lane = one env, SoA state, wave-uniform config through scalar loads):
//   kp1_step_kernel   action clip -> delta-q -> joint clip -> FK -> pose error -> zone counters ->
//                     termination -> reward -> state commit -> observation -> fused auto-reset
//                     (reference: KP1/envs/arm_kinematic_env.py:213-365 + callees, VecEnv auto-reset)
//   kp1_reset_kernel  reset(): explicit options or PCG64 sampling (arm_kinematic_env.py:102-211)
//   kp1_observe_kernel / kp1_fk_kernel / kp1_init_kernel / state gather-scatter helpers
//
// There is no CPU fallback: every entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/kp1_ppo.h"
#include "kp1_device.hpp"
#include "kp1_host.hpp"

using namespace kp1;

// ============================================================================================
// device code
// ============================================================================================
namespace {

#include "kp1_env_step.inc"

// POP (f32 only): a population handle.  Approach mode: env i auto-resets on the stage of tracker i / n_per_replica (kp1_bind_population_stages);
// dock mode: env i steps and resets with the live stage record of replica i / n_per_replica (kp1_dock_curriculum_create_population)
template <typename R, int MODE, bool COMPS, bool POP>
__global__ void __launch_bounds__(256, 1) kp1_step_kernel(const StepArgs<R> a) {
  extern __shared__ float obs_tiles[];   // OBS_TILE_FLOATS per wave of the workgroup
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
#ifdef KP1_ENV_TRACE   // slots 11 / 12: the chip-wide 100 MHz clock at wave entry / exit (the shader clock of slots 0..10 is not comparable across the chip)
  if ((threadIdx.x & 63) == 0 && (i >> 6) < KP1_ENV_TRACE_WAVES) kp1_env_trace_buf[(i >> 6) * KP1_ENV_TRACE_SLOTS + 11] = __builtin_amdgcn_s_memrealtime();
#endif
  const bool live = i < a.st.n;
  float o[KP1_OBS_DIM];
  if (live) step_env_lane<R, MODE, COMPS, POP>(a, i, a.actions + i * NJ, o);
  const int64_t i0 = i - (int64_t)(threadIdx.x & 63u);
  const int64_t left = a.st.n - i0;
  store_obs_tile(a.obs, i0, left >= 64 ? 64 : (left > 0 ? (int)left : 0), o, live, a.obs_stride, obs_tiles + (threadIdx.x >> 6) * OBS_TILE_FLOATS);
  KP1_ETR(8)
#ifdef KP1_ENV_TRACE
  __builtin_amdgcn_s_waitcnt(0);   // every store of this wave acknowledged
  KP1_ETR(9)
  if ((threadIdx.x & 63) == 0 && (i >> 6) < KP1_ENV_TRACE_WAVES) kp1_env_trace_buf[(i >> 6) * KP1_ENV_TRACE_SLOTS + 12] = __builtin_amdgcn_s_memrealtime();
#endif
}

// POP (f32 dock only): a dock population handle, env i samples with the live stage record pop_dock[i / n_per_replica] (the step's reset branch)
template <typename R, int MODE, bool POP = false>
__global__ void __launch_bounds__(256) kp1_reset_kernel(const EnvState<R> st, const DevCfg<R>* cfg, const DevSampler* smp, const kp1_handoff_state* handoff,
                                 const uint8_t* mask, const ResetOptsDev opts, int stage_index, float* obs, int obs_stride,
                                 const kp1_dock_curriculum_stage* pop_dock, int n_per_replica) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= st.n) return;
  if (mask && !mask[i]) return;
  float o[KP1_OBS_DIM];
  if constexpr (POP) {
    static_assert(MODE == KP1_MODE_DOCK, "the reset kernel's population form is the dock mode's");
    reset_env<R, MODE, true>(st, uniform_block(cfg), uniform_block(smp), handoff, opts, stage_index, i, o, pop_dock + (uint32_t)i / (uint32_t)n_per_replica);
  } else {
    reset_env<R, MODE>(st, uniform_block(cfg), uniform_block(smp), handoff, opts, stage_index, i, o);
  }
  if (obs) store_obs_row(obs, i, o, obs_stride);
}

template <typename R>
__global__ void kp1_observe_kernel(const EnvState<R> st, const DevCfg<R>* cfgp, int mode, float* obs, int obs_stride) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= st.n) return;
  const DevCfg<R>& cfg = *cfgp;
  R q[NJ], dq[NJ], pa[NJ], goal[6], ee[6], pe[3], oe[3], pn, on;
  for (int k = 0; k < NJ; ++k) {
    q[k] = st.r(F_Q + k, i);
    dq[k] = st.r(F_DQ + k, i);
    pa[k] = st.r(F_PREV_ACTION + k, i);
  }
  for (int k = 0; k < 6; ++k) {
    goal[k] = st.r(F_GOAL_POSE + k, i);
    ee[k] = st.r(F_EE_POSE + k, i);
  }
  pose_error_norms<R>(ee, goal, pe, oe, &pn, &on);
  float o[KP1_OBS_DIM];
  build_observation<R>(cfg, mode, q, dq, pa, pe, oe, st.iv(I_STEP, i), st.iv(I_DWELL, i), o);
  store_obs_row(obs, i, o, obs_stride);
}

// __init__: zero state, ee_pose6 = FK(0); arm_kinematic_env.py:80-100
template <typename R>
__global__ void __launch_bounds__(256) kp1_init_kernel(const EnvState<R> st, const DevCfg<R>* cfg) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= st.n) return;
  for (int f = 0; f < F_NUM_REAL; ++f) st.r(f, i) = (R)0;
  for (int f = 0; f < I_NUM_INT; ++f) st.iv(f, i) = 0;
  const double q[NJ] = {0, 0, 0, 0, 0, 0, 0};
  R ee[6];
  fk_pose6_kin<R>(cfg->kin.fk, q, ee);
  for (int k = 0; k < 6; ++k) st.r(F_EE_POSE + k, i) = ee[k];
  st.r(F_MIN_POS, i) = std::numeric_limits<R>::infinity();
}

template <typename R>
__global__ void kp1_fk_kernel(const DevFk<double>* fk, const R* q, R* pose, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double qq[NJ];
  R p[6];
  for (int k = 0; k < NJ; ++k) qq[k] = (double)q[i * NJ + k];
  fk_pose6_kin<R>(*fk, qq, p);
  for (int k = 0; k < 6; ++k) pose[i * 6 + k] = p[k];
}

template <typename R>
__global__ void kp1_pose_error_kernel(const R* curr, const R* goal, R* pos_err, R* ori_err, R* norms, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  R c[6], g[6], pe[3], oe[3], pn, on;
  for (int k = 0; k < 6; ++k) {
    c[k] = curr[i * 6 + k];
    g[k] = goal[i * 6 + k];
  }
  pose_error_norms<R>(c, g, pe, oe, &pn, &on);
  for (int k = 0; k < 3; ++k) {
    if (pos_err) pos_err[i * 3 + k] = pe[k];
    if (ori_err) ori_err[i * 3 + k] = oe[k];
  }
  if (norms) {
    norms[i * 2 + 0] = pn;
    norms[i * 2 + 1] = on;
  }
}

template <typename R>
struct JointLimitsDev { R lower[NJ], upper[NJ], dlim[NJ]; };

template <typename R>
__global__ void kp1_joint_utils_kernel(const JointLimitsDev<R> lim, const R* q, const R* dq, R* clipped, R* margin, R* q_norm, R* dq_norm, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int k = 0; k < NJ; ++k) {
    const R lo = lim.lower[k], hi = lim.upper[k];
    if (q) {
      const R c = joint_clip<R>(q[i * NJ + k], lo, hi);
      if (clipped) clipped[i * NJ + k] = c;
      if (margin) margin[i * NJ + k] = joint_limit_margin<R>(c, lo, hi);
      if (q_norm) q_norm[i * NJ + k] = joint_normalize_q<R>(q[i * NJ + k], lo, hi);
    }
    if (dq && dq_norm) dq_norm[i * NJ + k] = joint_normalize_dq<R>(dq[i * NJ + k], lim.dlim[k]);
  }
}

// set_state: scatter row-major fp64 host-provided rows into the SoA state, recompute ee = FK(q)
template <typename R>
__global__ void kp1_set_state_kernel(const EnvState<R> st, const DevCfg<R>* cfg, const double* q, const double* dq, const double* pa,
                                     const double* goal_q, const double* goal_pose, int capture_entry) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= st.n) return;
  if (q) {
    double qq[NJ];
    R ee[6];
    for (int k = 0; k < NJ; ++k) {
      qq[k] = q[i * NJ + k];
      st.q_store(k, i, qq[k]);
    }
    fk_pose6_kin<R>(cfg->kin.fk, qq, ee);
    for (int k = 0; k < 6; ++k) st.r(F_EE_POSE + k, i) = ee[k];
  }
  if (dq) for (int k = 0; k < NJ; ++k) st.r(F_DQ + k, i) = (R)dq[i * NJ + k];
  if (pa) for (int k = 0; k < NJ; ++k) st.r(F_PREV_ACTION + k, i) = (R)pa[i * NJ + k];
  if (goal_q) for (int k = 0; k < NJ; ++k) st.r(F_GOAL_Q + k, i) = (R)goal_q[i * NJ + k];
  if (goal_pose) for (int k = 0; k < 6; ++k) st.r(F_GOAL_POSE + k, i) = (R)goal_pose[i * 6 + k];
  // the error norms of the info view follow a moved pose whether or not the entry metrics are captured (_base_info computes them from the
  // current poses, arm_kinematic_env.py:385-387; kp1_eval_accumulate's step 0 reads them)
  if (capture_entry || q || goal_pose) {
    R ee[6], goal[6], pe[3], oe[3], pn, on, v[NJ];
    for (int k = 0; k < 6; ++k) {
      ee[k] = st.r(F_EE_POSE + k, i);
      goal[k] = st.r(F_GOAL_POSE + k, i);
    }
    pose_error_norms<R>(ee, goal, pe, oe, &pn, &on);
    st.r(F_POS_ERR, i) = pn;
    st.r(F_ORI_ERR, i) = on;
    if (capture_entry) {
      st.r(F_ENTRY + 0, i) = pn;
      st.r(F_ENTRY + 1, i) = on;
      for (int k = 0; k < NJ; ++k) v[k] = st.r(F_PREV_ACTION + k, i);
      st.r(F_ENTRY + 2, i) = norm7<R>(v);
      for (int k = 0; k < NJ; ++k) v[k] = st.r(F_DQ + k, i);
      st.r(F_ENTRY + 3, i) = norm7<R>(v);
    }
  }
}

template <typename R>
__global__ void kp1_get_state_kernel(const EnvState<R> st, double* q, double* dq, double* pa, double* goal_q, double* goal_pose) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= st.n) return;
  for (int k = 0; k < NJ; ++k) {
    if (q) q[i * NJ + k] = st.q_load(k, i);
    if (dq) dq[i * NJ + k] = (double)st.r(F_DQ + k, i);
    if (pa) pa[i * NJ + k] = (double)st.r(F_PREV_ACTION + k, i);
    if (goal_q) goal_q[i * NJ + k] = (double)st.r(F_GOAL_Q + k, i);
  }
  if (goal_pose) for (int k = 0; k < 6; ++k) goal_pose[i * 6 + k] = (double)st.r(F_GOAL_POSE + k, i);
}

}  // namespace

// ============================================================================================
// host side
// ============================================================================================
namespace {

// ---- numpy SeedSequence + PCG64 seeding (numpy/random/bit_generator.pyx, src/pcg64/pcg64.h) ----
uint32_t ss_hashmix(uint32_t value, uint32_t& hash_const) {
  value ^= hash_const;
  hash_const *= 0x931e8875u;
  value *= hash_const;
  value ^= value >> 16;
  return value;
}
uint32_t ss_mix(uint32_t x, uint32_t y) {
  uint32_t r = 0xca01f9ddu * x - 0x4973f715u * y;
  r ^= r >> 16;
  return r;
}
void pcg64_seed(uint64_t seed, kp1_rng_state* out) {
  uint32_t entropy[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
  const int n_ent = entropy[1] != 0 ? 2 : 1;
  uint32_t pool[4];
  uint32_t hc = 0x43b0d7e5u;
  for (int i = 0; i < 4; ++i) pool[i] = ss_hashmix(i < n_ent ? entropy[i] : 0u, hc);
  for (int s = 0; s < 4; ++s)
    for (int d = 0; d < 4; ++d)
      if (s != d) pool[d] = ss_mix(pool[d], ss_hashmix(pool[s], hc));
  uint32_t w[8];
  uint32_t hb = 0x8b51f9ddu;
  for (int i = 0; i < 8; ++i) {
    uint32_t v = pool[i & 3];
    v ^= hb;
    hb *= 0x58f38dedu;
    v *= hb;
    v ^= v >> 16;
    w[i] = v;
  }
  uint64_t s64[4];
  for (int i = 0; i < 4; ++i) s64[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
  const unsigned __int128 MULT = (((unsigned __int128)0x2360ED051FC65DA4ULL) << 64) | 0x4385DF649FCCF645ULL;
  unsigned __int128 initstate = ((unsigned __int128)s64[0] << 64) | s64[1];
  unsigned __int128 initseq = ((unsigned __int128)s64[2] << 64) | s64[3];
  unsigned __int128 inc = (initseq << 1) | 1u;
  unsigned __int128 state = 0;
  state = state * MULT + inc;
  state += initstate;
  state = state * MULT + inc;
  out->state_hi = (uint64_t)(state >> 64);
  out->state_lo = (uint64_t)state;
  out->inc_hi = (uint64_t)(inc >> 64);
  out->inc_lo = (uint64_t)inc;
  out->has_uint32 = 0;
  out->uinteger = 0;
}

// ---- FK constant folding in fp64 (V51/ee_fk.py:14-95) ----
const double ORIGIN_XYZ[7][3] = {
    {0.00715921043213119, 0.0000809621375843506, -0.0635},
    {-0.021178, 0.0, 0.1868},
    {-0.0633967414837172, 0.000642782425827271, 0.0602000000000009},
    {-0.000134989688424625, 0.425, 0.0133123982251372},
    {-0.0000850456535865796, -0.39225, -0.0083864861805065},
    {0.0475482889721905, -0.000817137634885778, -0.0805958577476871},
    {0.0436977540622506, 0.000443046177049933, -0.0521517110277254}};
const double ORIGIN_RPY[7][3] = {{0, 0, 0},
                                 {0, 0, 0},
                                 {1.5707963267949, 0.0, 1.5707963267949},
                                 {3.14159265358979, 0.0, 0.0},
                                 {3.14159265358979, 0.0, -1.5707963267949},
                                 {3.14159265358979, 1.5707963267949, 0.0},
                                 {-1.5707963267949, 0.0, -1.5707963267949}};
const double AXES_LOCAL[7][3] = {{1.0, 0.0, 0.0},
                                 {0.0, 0.0, 1.0},
                                 {0.0101382310641698, 0.0, -0.999948606814815},
                                 {0.010138231064165, 0.0, 0.999948606814815},
                                 {0.0, -0.0101382310641647, -0.999948606814815},
                                 {0.0, 0.0, -1.0},
                                 {-0.0101384515502096, 0.0, 0.999948604579338}};

void mat3_mul(const double* a, const double* b, double* c) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0;
      for (int k = 0; k < 3; ++k) s += a[3 * i + k] * b[3 * k + j];
      c[3 * i + j] = s;
    }
}
void rpy_to_rot(const double* rpy, double* R) {
  double cr = std::cos(rpy[0]), sr = std::sin(rpy[0]), cp = std::cos(rpy[1]), sp = std::sin(rpy[1]), cy = std::cos(rpy[2]), sy = std::sin(rpy[2]);
  double rx[9] = {1, 0, 0, 0, cr, -sr, 0, sr, cr};
  double ry[9] = {cp, 0, sp, 0, 1, 0, -sp, 0, cp};
  double rz[9] = {cy, -sy, 0, sy, cy, 0, 0, 0, 1};
  double t[9];
  mat3_mul(rz, ry, t);
  mat3_mul(t, rx, R);
}
template <typename R>
void fold_fk(DevFk<R>* out) {
  double RA[7][9];
  for (int i = 0; i < 7; ++i) rpy_to_rot(ORIGIN_RPY[i], RA[i]);
  // prismatic joint 0: p = p0 + RA0 (a0 q0); then origin of joint 1: p += RA0 p1
  double a0n = std::sqrt(AXES_LOCAL[0][0] * AXES_LOCAL[0][0] + AXES_LOCAL[0][1] * AXES_LOCAL[0][1] + AXES_LOCAL[0][2] * AXES_LOCAL[0][2]);
  (void)a0n;  // the reference does NOT normalise the prismatic axis (ee_fk.py:113)
  for (int r = 0; r < 3; ++r) {
    double v = 0, pp = ORIGIN_XYZ[0][r];
    for (int k = 0; k < 3; ++k) {
      v += RA[0][3 * r + k] * AXES_LOCAL[0][k];
      pp += RA[0][3 * r + k] * ORIGIN_XYZ[1][k];
    }
    out->v0[r] = (R)v;
    out->p01[r] = (R)pp;
  }
  for (int j = 1; j < 7; ++j) {
    const double* ax = AXES_LOCAL[j];
    double nrm = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) + 1e-12;  // ee_fk.py:76
    double x = ax[0] / nrm, y = ax[1] / nrm, z = ax[2] / nrm;
    double aat[9] = {x * x, x * y, x * z, y * x, y * y, y * z, z * x, z * y, z * z};
    double skew[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    double eye_m[9];
    for (int e = 0; e < 9; ++e) eye_m[e] = ((e % 4 == 0) ? 1.0 : 0.0) - aat[e];
    double base[9];
    if (j == 1) mat3_mul(RA[0], RA[1], base);  // fold the (rotation of the) prismatic stage into joint 1
    else std::memcpy(base, RA[j], sizeof base);
    double k1[9], kc[9], ks[9];
    mat3_mul(base, aat, k1);
    mat3_mul(base, eye_m, kc);
    mat3_mul(base, skew, ks);
    for (int e = 0; e < 9; ++e) {
      out->k1[j - 1][e] = (R)k1[e];
      out->kc[j - 1][e] = (R)kc[e];
      out->ks[j - 1][e] = (R)ks[e];
    }
    if (j >= 2)
      for (int r = 0; r < 3; ++r) out->p[j - 2][r] = (R)ORIGIN_XYZ[j][r];
  }
}

#define KP1_CONV(type, name, dflt) d.name = (decltype(d.name))s.name;
template <typename R>
void make_dev_cfg(const kp1_config& c, DevCfg<R>* out) {
  std::memset(out, 0, sizeof *out);
  { auto& d = out->env; const auto& s = c.env; KP1_ENV_FIELDS(KP1_CONV) }
  { auto& d = out->reward; const auto& s = c.reward; KP1_APPROACH_REWARD_FIELDS(KP1_CONV) }
  { auto& d = out->dock; const auto& s = c.dock_reward; KP1_DOCK_REWARD_FIELDS(KP1_CONV) }
  { auto& d = out->term; const auto& s = c.termination; KP1_TERMINATION_FIELDS(KP1_CONV) }
  { auto& d = out->obs; const auto& s = c.observation; KP1_OBSERVATION_FIELDS(KP1_CONV) }
  for (int i = 0; i < KP1_MAX_MILESTONES; ++i) {
    out->reward.ms_thr[i] = (R)c.reward.orientation_milestone_thresholds_rad[i];
    out->reward.ms_bonus[i] = (R)c.reward.orientation_milestone_bonuses[i];
  }
  for (int i = 0; i < NJ; ++i) {
    out->lower[i] = (R)c.joints.lower[i];
    out->upper[i] = (R)c.joints.upper[i];
    out->dlim[i] = (R)c.joints.delta_limit[i];
    out->kin.lower[i] = c.joints.lower[i];
    out->kin.upper[i] = c.joints.upper[i];
    out->kin.dlim[i] = c.joints.delta_limit[i];
  }
  out->kin.action_delta_scale = c.env.action_delta_scale;
  out->kin.dock_action_delta_scale = c.env.dock_action_delta_scale;
  fold_fk<double>(&out->kin.fk);
}
void make_dev_sampler(const kp1_config& c, int n_handoff, DevSampler* s) {
  std::memset(s, 0, sizeof *s);
  for (int i = 0; i < NJ; ++i) {
    s->lower[i] = c.joints.lower[i];
    s->upper[i] = c.joints.upper[i];
  }
  s->curriculum_enabled = c.curriculum_enabled;
  s->n_stages = c.n_stages;
  std::memcpy(s->stages, c.stages, sizeof c.stages);
  s->ss = c.stage_sampling;
  s->rs = c.random_start;
  s->dr = c.dock_reset;
  s->start_sample_margin_fraction = c.env.start_sample_margin_fraction;
  s->goal_sample_margin_fraction = c.env.goal_sample_margin_fraction;
  s->n_handoff = n_handoff;
  s->handoff_offset = 0;
  fold_fk<double>(&s->fk);
}

#define KP1_SETD(type, name, dflt) s.name = dflt;
void config_default(kp1_config* cfg) {
  std::memset(cfg, 0, sizeof *cfg);
  { auto& s = cfg->env; KP1_ENV_FIELDS(KP1_SETD) }
  { auto& s = cfg->reward; KP1_APPROACH_REWARD_FIELDS(KP1_SETD) }
  { auto& s = cfg->dock_reward; KP1_DOCK_REWARD_FIELDS(KP1_SETD) }
  { auto& s = cfg->termination; KP1_TERMINATION_FIELDS(KP1_SETD) }
  { auto& s = cfg->observation; KP1_OBSERVATION_FIELDS(KP1_SETD) }
  { auto& s = cfg->stage_sampling; KP1_STAGE_SAMPLING_FIELDS(KP1_SETD) }
  { auto& s = cfg->random_start; KP1_RANDOM_START_FIELDS(KP1_SETD) }
  { auto& s = cfg->dock_reset; KP1_DOCK_RESET_FIELDS(KP1_SETD) }
  const double PI = 3.141592653589793;
  const double lim[NJ] = {0.385, PI, PI, PI, PI, PI, PI};              // KP1/kinematics/joint_limits.py:37-47
  const double dl[NJ] = {0.08, 0.30, 0.24, 0.24, 0.30, 0.40, 0.30};
  for (int i = 0; i < NJ; ++i) {
    cfg->joints.lower[i] = -lim[i];
    cfg->joints.upper[i] = lim[i];
    cfg->joints.delta_limit[i] = dl[i];
    cfg->random_start.failure_recovery_q_noise[i] = 0.04;
  }
  const double gn[NJ] = {0.01, 0.03, 0.04, 0.03, 0.02, 0.02, 0.01};   // KP1/envs/reset_samplers.py:50-54
  const double iq[NJ] = {0.01, 0.02, 0.03, 0.02, 0.015, 0.015, 0.01};
  const double cq[NJ] = {0.006, 0.012, 0.018, 0.012, 0.009, 0.009, 0.006};
  std::memcpy(cfg->dock_reset.goal_noise, gn, sizeof gn);
  std::memcpy(cfg->dock_reset.init_q_noise, iq, sizeof iq);
  std::memcpy(cfg->dock_reset.close_init_q_noise, cq, sizeof cq);
  const double goal_noise[6][NJ] = {{0.01, 0.03, 0.04, 0.03, 0.02, 0.02, 0.01}, {0.02, 0.06, 0.08, 0.06, 0.04, 0.04, 0.03},
                                    {0.03, 0.09, 0.12, 0.09, 0.06, 0.05, 0.04}, {0.04, 0.12, 0.16, 0.12, 0.08, 0.06, 0.05},
                                    {0.05, 0.14, 0.18, 0.14, 0.09, 0.07, 0.06}, {0.06, 0.18, 0.22, 0.16, 0.10, 0.08, 0.07}};
  const double start_noise[6] = {0.0, 0.0, 0.0, 0.01, 0.02, 0.03};      // KP1/envs/curriculum.py:36-78
  const double goal4[NJ] = {0.03, -0.04, 0.05, -0.03, 0.02, -0.01, 0.01};
  cfg->curriculum_enabled = 1;
  cfg->n_stages = 6;
  for (int k = 0; k < 6; ++k) {
    std::memcpy(cfg->stages[k].goal_noise, goal_noise[k], sizeof goal_noise[k]);
    for (int i = 1; i < NJ; ++i) cfg->stages[k].start_noise[i] = start_noise[k];
  }
  std::memcpy(cfg->stages[4].goal_q, goal4, sizeof goal4);
}

}  // namespace

struct kp1_env {
  kp1_config cfg;
  int32_t n = 0, device = 0, real_type = 0, stage = 0, mode = 0;
  hipStream_t stream = nullptr;
  void* real = nullptr;        // R[F_NUM_REAL][N]
  int32_t* ints = nullptr;     // [I_NUM_INT][N]
  uint64_t* rng64 = nullptr;   // [4][N]
  uint32_t* rng32 = nullptr;   // [2][N]
  void* dev_cfg = nullptr;     // DevCfg<R>
  DevSampler* dev_smp = nullptr;
  kp1_handoff_state* dev_handoff = nullptr;
  int32_t n_handoff = 0;
  // kp1_set_route_stride_reset: the live table and the host mirror of its scalars (upload_cfg writes them into every new DevSampler).
  // A replaced table stays allocated until kp1_destroy: a launch already queued may still read it.
  struct RouteStride {
    double* dev_q = nullptr;
    int32_t n_points = 0, n_min = 0, n_max = 0;
    int32_t min_stride[KP1_MAX_STAGES] = {}, max_stride[KP1_MAX_STAGES] = {};
    double start_noise[KP1_NJ] = {}, goal_noise[KP1_NJ] = {};
    double reverse_probability = 0.0;
  } route_stride;
  std::vector<double*> route_tables;   // every table ever uploaded, the live one included
  void* snapshot = nullptr;   // kp1_state_snapshot: real | ints | rng64 | rng32, allocated on first use
  kp1_dock_curriculum_state* dock_tracker = nullptr;   // device tracker attached by kp1_dock_curriculum_create (its stage survives upload_cfg)
  double* opt_scratch = nullptr;  // 4*[N][7] + [N][6] doubles for explicit reset options / set_state
  const int32_t* stage_ptr = nullptr;  // kp1_bind_stage_ptr
  const kp1_curriculum_state* pop_states = nullptr;   // kp1_bind_population_stages: K trackers, env i on tracker i / (n / pop_replicas)
  kp1_dock_curriculum_state* pop_dock_states = nullptr;   // kp1_dock_curriculum_create_population: K trackers, then their K live stage records
  int32_t pop_replicas = 0;   // K of whichever population is bound
  int32_t obs_stride = KP1_OBS_DIM;    // kp1_set_obs_stride
  void* comps = nullptr;          // R[64][N] when enabled
  bool comps_enabled = false;
  size_t real_size() const { return real_type == KP1_REAL_F64 ? 8 : 4; }
};

namespace {

// One wave per workgroup at every size: the step kernel holds 500 vector registers, so a CU runs four waves (one per SIMD), and a 256-thread
// workgroup can only be replaced when all four of its waves have finished.  64-thread workgroups let every SIMD take its next wave by itself:
// 117.5 -> 99.1 us at 524 288 envs, 33.8 -> 31.3 us at 131 072 (profiles/r03_ab_env_block_size.log).
constexpr int ENV_BLOCK = 64;
// The stateless utilities and eval_accumulate hold a few dozen registers per lane, so nothing waits on a workgroup's slowest wave: they keep the
// usual four waves per workgroup (eval_accumulate_kernel computes its lane from a block of 256).
constexpr int UTIL_BLOCK = 256;

// The one launch of this file: ceil(lanes / block) workgroups of `block` lanes, then the launch check of kp1_host.hpp.  `lanes` is the env
// count where a lane is an env; the curriculum trackers run one 64-lane wave each (lanes = 64 * trackers, block = 64).
template <typename... Params, typename... Args>
int launch_env(void (*kernel)(Params...), int64_t lanes, int block, size_t lds_bytes, hipStream_t stream, const Args&... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((lanes + block - 1) / block)), dim3(block), lds_bytes, stream, args...);
  HIP_TRY(kp1::launch_status());
  return KP1_OK;
}

// real_type -> the type itself: f(R()) with R = double or float, anything else refused.  The return types are deduced, here and in the callables
// (write no `-> int` on them): the bodies are then instantiated where with_real is called and not at the end of the file, so the kernels a callable
// names are first named at the call, in file order, which is what decides their place in the code object (DESIGN.md sections 26 and 41).
template <class F>
auto with_real(int real_type, F&& f) {
  if (real_type == KP1_REAL_F64) return f(double());
  if (real_type == KP1_REAL_F32) return f(float());
  return fail(KP1_ERR_INVALID, "real_type must be KP1_REAL_F32 or KP1_REAL_F64");
}

template <typename R>
EnvState<R> state_of(const kp1_env* e) {
  EnvState<R> st;
  st.real = (R*)e->real;
  st.ints = e->ints;
  st.rng64 = e->rng64;
  st.rng32 = e->rng32;
  st.n = e->n;
  return st;
}

int reapply_dock_stage(kp1_env* env);   // kp1_dock_curriculum.inc

int upload_cfg(kp1_env* e) {
  DevSampler s;
  make_dev_sampler(e->cfg, e->n_handoff, &s);
  {
    const kp1_env::RouteStride& r = e->route_stride;
    s.route_q = r.dev_q;
    s.route_points = r.n_points;
    s.route_n_min = r.n_min;
    s.route_n_max = r.n_max;
    std::memcpy(s.route_min_stride, r.min_stride, sizeof r.min_stride);
    std::memcpy(s.route_max_stride, r.max_stride, sizeof r.max_stride);
    std::memcpy(s.route_start_noise, r.start_noise, sizeof r.start_noise);
    std::memcpy(s.route_goal_noise, r.goal_noise, sizeof r.goal_noise);
    s.route_reverse_probability = r.reverse_probability;
  }
  const int rc = with_real(e->real_type, [&](auto real) {
    DevCfg<decltype(real)> d;
    make_dev_cfg(e->cfg, &d);
    HIP_TRY(hipMemcpyAsync(e->dev_cfg, &d, sizeof d, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->dev_smp, &s, sizeof s, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));  // d / s are stack objects
    return (int)KP1_OK;
  });
  return rc != KP1_OK ? rc : reapply_dock_stage(e);
}

// ---- the PCG64 streams of N envs on the device: [4][N] u64 (state_hi, state_lo, inc_hi, inc_lo) + [2][N] u32 (has_uint32, uinteger) ----
void pack_rng_planes(const kp1_rng_state* rows, size_t n, std::vector<uint64_t>& r64, std::vector<uint32_t>& r32) {
  r64.resize(4 * n);
  r32.resize(2 * n);
  for (size_t i = 0; i < n; ++i) {
    r64[0 * n + i] = rows[i].state_hi; r64[1 * n + i] = rows[i].state_lo; r64[2 * n + i] = rows[i].inc_hi; r64[3 * n + i] = rows[i].inc_lo;
    r32[0 * n + i] = rows[i].has_uint32; r32[1 * n + i] = rows[i].uinteger;
  }
}
void unpack_rng_planes(const std::vector<uint64_t>& r64, const std::vector<uint32_t>& r32, size_t n, kp1_rng_state* rows) {
  for (size_t i = 0; i < n; ++i) {
    rows[i].state_hi = r64[0 * n + i]; rows[i].state_lo = r64[1 * n + i]; rows[i].inc_hi = r64[2 * n + i]; rows[i].inc_lo = r64[3 * n + i];
    rows[i].has_uint32 = r32[0 * n + i]; rows[i].uinteger = r32[1 * n + i];
  }
}
int upload_rng_planes(uint64_t* dst64, uint32_t* dst32, const kp1_rng_state* rows, size_t n, hipStream_t stream) {
  std::vector<uint64_t> r64;
  std::vector<uint32_t> r32;
  pack_rng_planes(rows, n, r64, r32);
  HIP_TRY(hipMemcpyAsync(dst64, r64.data(), r64.size() * 8, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(dst32, r32.data(), r32.size() * 4, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return KP1_OK;
}
int download_rng_planes(const uint64_t* src64, const uint32_t* src32, kp1_rng_state* rows, size_t n, hipStream_t stream) {
  std::vector<uint64_t> r64(4 * n);
  std::vector<uint32_t> r32(2 * n);
  HIP_TRY(hipMemcpyAsync(r64.data(), src64, r64.size() * 8, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(r32.data(), src32, r32.size() * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  unpack_rng_planes(r64, r32, n, rows);
  return KP1_OK;
}
// stream i <- default_rng(seed_of(i))
template <typename SeedOf>
int seed_planes_by(uint64_t* dst64, uint32_t* dst32, int64_t n, hipStream_t stream, SeedOf seed_of) {
  std::vector<kp1_rng_state> rows((size_t)n);
  for (int64_t i = 0; i < n; ++i) pcg64_seed(seed_of(i), &rows[(size_t)i]);
  return upload_rng_planes(dst64, dst32, rows.data(), rows.size(), stream);
}
template <typename SeedOf>
int seed_streams_by(kp1_env* e, SeedOf seed_of) {
  return seed_planes_by(e->rng64, e->rng32, e->n, e->stream, seed_of);
}

int seed_streams(kp1_env* e, uint64_t seed0, uint64_t first_env_id) {
  return seed_streams_by(e, [=](int64_t i) { return seed0 + first_env_id + (uint64_t)i; });
}

// the K live stage records of a bound dock population (kp1_dock_curriculum_create_population), or nullptr
const kp1_dock_curriculum_stage* dock_population_live(const kp1_env* e) {
  return e->pop_dock_states ? reinterpret_cast<const kp1_dock_curriculum_stage*>(e->pop_dock_states + e->pop_replicas) : nullptr;
}

template <typename R>
StepArgs<R> make_step_args(kp1_env* e, const void* actions, float* obs, void* reward, uint8_t* done, float* terminal_obs, int auto_reset) {
  StepArgs<R> a;
  a.st = state_of<R>(e);
  a.cfg = (const DevCfg<R>*)e->dev_cfg;
  a.smp = e->dev_smp;
  a.handoff = e->dev_handoff;
  a.actions = (const R*)actions;
  a.obs = obs;
  a.reward = (R*)reward;
  a.done = done;
  a.terminal_obs = terminal_obs;
  a.comps = (R*)e->comps;
  a.auto_reset = auto_reset;
  a.stage_index = e->stage;
  a.obs_stride = e->obs_stride;
  a.stage_ptr = e->cfg.curriculum_enabled ? e->stage_ptr : nullptr;
  a.pop_states = e->pop_states;
  a.n_per_replica = e->pop_replicas > 0 ? e->n / e->pop_replicas : 0;
  a.pop_dock = dock_population_live(e);
  return a;
}

template <typename R>
int launch_step(kp1_env* e, const void* actions, float* obs, void* reward, uint8_t* done, float* terminal_obs, int auto_reset) {
  const StepArgs<R> a = make_step_args<R>(e, actions, obs, reward, done, terminal_obs, auto_reset);
  const bool comps = e->comps_enabled && e->comps;
  constexpr bool F32 = std::is_same<R, float>::value;
  // the eight (MODE, COMPS, POP) forms share a signature: choose one (first named here = first in the code object), launch once
  void (*kernel)(const StepArgs<R>) = nullptr;
  if (e->pop_dock_states || e->pop_states) {
    // Per-replica stages exist as f32 forms only: the dock form for a dock population, the approach form for bound approach trackers (the two
    // creators check type and mode; kp1_set_mode may change the mode later).  Approach without curriculum stages never reads the stage, and
    // the ordinary form below does the same work.
    if (e->pop_dock_states && e->mode != KP1_MODE_DOCK) return fail(KP1_ERR_UNSUPPORTED, "a dock population env handle steps in the dock mode only");
    if (!e->pop_dock_states && e->mode != KP1_MODE_APPROACH) return fail(KP1_ERR_UNSUPPORTED, "a population env handle steps in the approach mode only");
    if constexpr (!F32) return fail(KP1_ERR_UNSUPPORTED, "a population env handle is f32");
    else if (e->pop_dock_states) kernel = comps ? kp1_step_kernel<float, KP1_MODE_DOCK, true, true> : kp1_step_kernel<float, KP1_MODE_DOCK, false, true>;
    else if (e->cfg.curriculum_enabled) kernel = comps ? kp1_step_kernel<float, KP1_MODE_APPROACH, true, true> : kp1_step_kernel<float, KP1_MODE_APPROACH, false, true>;
  }
  if (!kernel) {
    if (e->mode == KP1_MODE_DOCK) kernel = comps ? kp1_step_kernel<R, KP1_MODE_DOCK, true, false> : kp1_step_kernel<R, KP1_MODE_DOCK, false, false>;
    else kernel = comps ? kp1_step_kernel<R, KP1_MODE_APPROACH, true, false> : kp1_step_kernel<R, KP1_MODE_APPROACH, false, false>;
  }
  const size_t lds = sizeof(float) * OBS_TILE_FLOATS * (size_t)(ENV_BLOCK / 64);   // one observation tile per wave (store_obs_tile)
  return launch_env(kernel, e->n, ENV_BLOCK, lds, e->stream, a);
}

template <typename R>
int launch_reset(kp1_env* e, const uint8_t* mask, const ResetOptsDev& opts, int mode, float* obs) {
  // a dock population samples each replica's resets with its own live stage (the shared config holds stage 0 only)
  const kp1_dock_curriculum_stage* live = mode == KP1_MODE_DOCK ? dock_population_live(e) : nullptr;
  decltype(&kp1_reset_kernel<R, KP1_MODE_DOCK>) kernel;   // the three forms share a signature
  if (live) {
    if constexpr (std::is_same<R, float>::value) kernel = kp1_reset_kernel<float, KP1_MODE_DOCK, true>;
    else return fail(KP1_ERR_UNSUPPORTED, "a population env handle is f32");
  } else if (mode == KP1_MODE_DOCK) {
    kernel = kp1_reset_kernel<R, KP1_MODE_DOCK>;
  } else {
    kernel = kp1_reset_kernel<R, KP1_MODE_APPROACH>;
  }
  return launch_env(kernel, e->n, ENV_BLOCK, 0, e->stream, state_of<R>(e), (const DevCfg<R>*)e->dev_cfg, e->dev_smp, e->dev_handoff, mask, opts, e->stage, obs,
                    e->obs_stride, live, live ? e->n / e->pop_replicas : 0);
}

// ---------------------------------------------------------------------------------------------- evaluator bookkeeping (kp1_eval_accumulate)
// One lane per episode.  The bookkeeping of a step (step >= 1) is eval_account_step, shared with eval_step_kernel (kp1_eval_step.inc).
#include "kp1_eval_account.inc"
template <typename R>
__global__ void __launch_bounds__(256) eval_accumulate_kernel(const R* __restrict__ real, int n, kp1_eval_buffers b, const double* __restrict__ action_norm,
                                                              const uint8_t* __restrict__ done, const uint8_t* __restrict__ active, int step, bool track_ready,
                                                              double thr_pos, double thr_ori, double thr_act, double thr_dq, int confirm) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int alive_after = 0;
  if (i < n) {
    double* M = b.metrics;
    int32_t* C = b.counters;
    uint8_t* F = b.flags;
    const double pos = (double)real[(size_t)F_POS_ERR * n + i], ori = (double)real[(size_t)F_ORI_ERR * n + i];
    if (step == 0) {
      M[0 * (size_t)n + i] = pos; M[1 * (size_t)n + i] = ori; M[2 * (size_t)n + i] = pos; M[3 * (size_t)n + i] = ori;
      for (int k = 4; k < 8; ++k) M[k * (size_t)n + i] = 0.0;
      C[0 * (size_t)n + i] = 0; C[1 * (size_t)n + i] = 0; C[2 * (size_t)n + i] = -1; C[3 * (size_t)n + i] = 0;
      const uint8_t a = active ? (active[i] ? 1 : 0) : 1;
      F[0 * (size_t)n + i] = a; F[1 * (size_t)n + i] = 0; F[2 * (size_t)n + i] = 0; F[3 * (size_t)n + i] = 0;
      for (int f = 0; f < EVAL_STATE_W; ++f) b.state[(size_t)i * EVAL_STATE_W + f] = (double)real[(size_t)f * n + i];
      if (b.hand_metrics) {
        for (int k = 0; k < 8; ++k) b.hand_metrics[k * (size_t)n + i] = 0.0;
        b.hand_step[i] = 0;
        b.hand_success[i] = 0;
        for (int f = 0; f < EVAL_STATE_W; ++f) b.hand_state[(size_t)i * EVAL_STATE_W + f] = 0.0;
      }
      alive_after = a;
    } else {
      alive_after = eval_account_step<R>(real, n, i, b, action_norm[i], done[i], step, track_ready, thr_pos, thr_ori, thr_act, thr_dq, confirm);
    }
  }
  // episodes still alive: wave ballot, one atomic per wave (an integer count: order does not matter)
  const unsigned long long bal = __ballot(alive_after != 0);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(b.n_alive, __popcll(bal));
}

// opt_scratch: five row-major fp64 blocks, one per optional array of kp1_reset_opts / kp1_set_state / kp1_get_state, in their order
// (q, dq, prev_action, goal_q: [N][7]; goal_pose6: [N][6]).  Allocated on first use.
struct OptScratch {
  double* dev[5];
  size_t bytes[5];
};
int ensure_scratch(kp1_env* e, OptScratch* s) {
  const int width[5] = {NJ, NJ, NJ, NJ, 6};
  size_t total = 0;
  for (int k = 0; k < 5; ++k) total += s->bytes[k] = sizeof(double) * (size_t)e->n * width[k];
  if (!e->opt_scratch) HIP_TRY(hipMalloc((void**)&e->opt_scratch, total));
  s->dev[0] = e->opt_scratch;
  for (int k = 1; k < 5; ++k) s->dev[k] = s->dev[k - 1] + (size_t)e->n * width[k - 1];
  return KP1_OK;
}
// the rows the caller gave (src[k], host) into their blocks; dev[k] = the block, or nullptr where src[k] is
int upload_opt_rows(kp1_env* e, const double* const src[5], const double* dev[5]) {
  OptScratch s;
  const int rc = ensure_scratch(e, &s);
  if (rc != KP1_OK) return rc;
  for (int k = 0; k < 5; ++k) {
    dev[k] = src[k] ? s.dev[k] : nullptr;
    if (src[k]) HIP_TRY(hipMemcpyAsync(s.dev[k], src[k], s.bytes[k], hipMemcpyHostToDevice, e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));  // host source buffers are the caller's
  return KP1_OK;
}

}  // namespace

// ============================================================================================
// C ABI
// ============================================================================================
namespace kp1 {
int env_step_args_f32_population(kp1_env* e, void* out, size_t out_bytes, float* obs, void* reward, uint8_t* done, float* terminal_obs,
                                 int auto_reset, int* mode, int64_t* n_envs, int* device, int* pop_replicas, int* pop_form) {
  if (!e || !out) return fail(KP1_ERR_INVALID, "NULL argument");
  if (e->real_type != KP1_REAL_F32) return fail(KP1_ERR_UNSUPPORTED, "the fused policy + env step runs on the fp32 handle");
  if (e->comps_enabled && e->comps) return fail(KP1_ERR_UNSUPPORTED, "the fused policy + env step does not record reward components");
  if (out_bytes != sizeof(StepArgs<float>)) return fail(KP1_ERR_INVALID, "StepArgs<float> layout mismatch between translation units");
  // the forms launch_step chooses between
  if (e->pop_dock_states && e->mode != KP1_MODE_DOCK) return fail(KP1_ERR_UNSUPPORTED, "a dock population env handle steps in the dock mode only");
  if (e->pop_states && e->mode != KP1_MODE_APPROACH) return fail(KP1_ERR_UNSUPPORTED, "a population env handle steps in the approach mode only");
  const StepArgs<float> a = make_step_args<float>(e, nullptr, obs, reward, done, terminal_obs, auto_reset);
  std::memcpy(out, &a, sizeof a);
  *mode = e->mode;
  *n_envs = e->n;
  *device = e->device;
  *pop_replicas = (e->pop_dock_states || e->pop_states) ? e->pop_replicas : 0;
  *pop_form = (e->pop_dock_states || (e->pop_states && e->cfg.curriculum_enabled)) ? 1 : 0;
  return KP1_OK;
}

int env_step_args_f32(kp1_env* e, void* out, size_t out_bytes, const void* actions, float* obs, void* reward, uint8_t* done, float* terminal_obs,
                      int auto_reset, int* mode, int64_t* n_envs, int* device) {
  if (!e || !out) return fail(KP1_ERR_INVALID, "NULL argument");
  if (e->real_type != KP1_REAL_F32) return fail(KP1_ERR_UNSUPPORTED, "the fused policy + env step runs on the fp32 handle");
  if (e->comps_enabled && e->comps) return fail(KP1_ERR_UNSUPPORTED, "the fused policy + env step does not record reward components");
  if (e->pop_states) return fail(KP1_ERR_UNSUPPORTED, "the fused policy + env step has no per-replica stage (population env handle)");
  if (e->pop_dock_states) return fail(KP1_ERR_UNSUPPORTED, "the fused policy + env step has no per-replica dock stage (dock population env handle)");
  int pop_replicas = 0, pop_form = 0;   // both 0: the population refusals above
  const int rc = env_step_args_f32_population(e, out, out_bytes, obs, reward, done, terminal_obs, auto_reset, mode, n_envs, device, &pop_replicas, &pop_form);
  if (rc == KP1_OK) static_cast<StepArgs<float>*>(out)->actions = (const float*)actions;
  return rc;
}

void env_bound_stage_source(const kp1_env* e, const void** stage_ptr, const void** pop_states) {
  *stage_ptr = e->stage_ptr;
  *pop_states = e->pop_states;
}
}  // namespace kp1

extern "C" {

const char* kp1_last_error(void) { return g_last_error.c_str(); }
int kp1_abi_version(void) { return 1; }
uint64_t kp1_config_size(void) { return sizeof(kp1_config); }
int kp1_config_default(kp1_config* cfg) {
  if (!cfg) return fail(KP1_ERR_INVALID, "cfg is NULL");
  config_default(cfg);
  return KP1_OK;
}
int kp1_rng_seed_state(uint64_t seed, kp1_rng_state* out) {
  if (!out) return fail(KP1_ERR_INVALID, "out is NULL");
  pcg64_seed(seed, out);
  return KP1_OK;
}

int kp1_create(const kp1_config* cfg, int32_t n_envs, int32_t device, int32_t real_type, uint64_t seed0, uint64_t first_env_id,
               void* stream, kp1_env** out) {
  if (!cfg || !out) return fail(KP1_ERR_INVALID, "cfg/out is NULL");
  if (n_envs <= 0) return fail(KP1_ERR_INVALID, "n_envs must be positive");
  if (n_envs > (1 << 22)) return fail(KP1_ERR_INVALID, "n_envs above 2^22: a lane's byte offset inside the state arrays ((field * n + env) * 8) must fit 32 bits");
  if (real_type != KP1_REAL_F32 && real_type != KP1_REAL_F64) return fail(KP1_ERR_INVALID, "real_type must be KP1_REAL_F32 or KP1_REAL_F64");
  if (cfg->env.mode != KP1_MODE_APPROACH && cfg->env.mode != KP1_MODE_DOCK) return fail(KP1_ERR_UNSUPPORTED, "mode must be approach or dock");
  if (cfg->n_stages < 0 || cfg->n_stages > KP1_MAX_STAGES) return fail(KP1_ERR_INVALID, "n_stages out of range");
  if (cfg->curriculum_enabled && cfg->n_stages == 0) return fail(KP1_ERR_INVALID, "curriculum enabled without stages");
  if (cfg->reward.n_orientation_milestones < 0 || cfg->reward.n_orientation_milestones > KP1_MAX_MILESTONES)
    return fail(KP1_ERR_INVALID, "n_orientation_milestones out of range");
  {   // the fp32 handle's generated FK chain carries the robot constants as literals: they must be what fold_fk computes here, bit for bit
    DevFk<double> fk;
    fold_fk<double>(&fk);
    static_assert(sizeof(DevFk<double>) == sizeof(FKG_CHECK), "FKG_CHECK lists DevFk<double> member by member");
    if (std::memcmp(&fk, FKG_CHECK, sizeof fk) != 0)
      return fail(KP1_ERR_UNSUPPORTED, "csrc/kp1_fk_generated.inc does not match the robot constants of kp1_env.hip: run python3 tools/gen_fk_chain.py and rebuild");
  }
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  kp1_env* e = new kp1_env();
  e->cfg = *cfg;
  e->n = n_envs;
  e->device = device;
  e->real_type = real_type;
  e->stream = (hipStream_t)stream;
  e->mode = cfg->env.mode;
  e->stage = 0;
  const size_t n = (size_t)n_envs;
  auto cleanup = [&]() { kp1_destroy(e); };
#define KP1_ALLOC(ptr, bytes)                                   \
  if (hipMalloc((void**)&(ptr), (bytes)) != hipSuccess) {       \
    cleanup();                                                  \
    return fail(KP1_ERR_ALLOC, "hipMalloc failed for " #ptr);   \
  }
  KP1_ALLOC(e->real, e->real_size() * F_NUM_REAL * n);
  KP1_ALLOC(e->ints, sizeof(int32_t) * I_NUM_INT * n);
  KP1_ALLOC(e->rng64, sizeof(uint64_t) * 4 * n);
  KP1_ALLOC(e->rng32, sizeof(uint32_t) * 2 * n);
  KP1_ALLOC(e->dev_cfg, ((real_type == KP1_REAL_F64 ? sizeof(DevCfg<double>) : sizeof(DevCfg<float>)) + KP1_WARM_BYTES - 1) / KP1_WARM_BYTES * KP1_WARM_BYTES);
  KP1_ALLOC(e->dev_smp, sizeof(DevSampler));
#undef KP1_ALLOC
  rc = upload_cfg(e);
  if (rc == KP1_OK) rc = seed_streams(e, seed0, first_env_id);
  if (rc == KP1_OK)
    rc = with_real(real_type, [&](auto real) {
      using R = decltype(real);
      return launch_env(kp1_init_kernel<R>, e->n, ENV_BLOCK, 0, e->stream, state_of<R>(e), (const DevCfg<R>*)e->dev_cfg);
    });
  if (rc != KP1_OK) {
    cleanup();
    return rc;
  }
  *out = e;
  return KP1_OK;
}

int kp1_destroy(kp1_env* e) {
  if (!e) return KP1_OK;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  else (void)hipDeviceSynchronize();
  for (void* p : {(void*)e->real, (void*)e->ints, (void*)e->rng64, (void*)e->rng32, e->dev_cfg, (void*)e->dev_smp, (void*)e->dev_handoff,
                  (void*)e->opt_scratch, e->comps, e->snapshot})
    (void)hipFree(p);
  for (double* p : e->route_tables) (void)hipFree(p);
  delete e;
  return KP1_OK;
}

int kp1_num_envs(const kp1_env* e) { return e ? e->n : 0; }

int kp1_set_stage(kp1_env* e, int32_t stage_index) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  if (!e->cfg.curriculum_enabled) return KP1_OK;  // arm_kinematic_env.py:447-448
  int hi = e->cfg.n_stages - 1;
  e->stage = stage_index < 0 ? 0 : (stage_index > hi ? hi : stage_index);
  return KP1_OK;
}
int kp1_bind_stage_ptr(kp1_env* e, const int32_t* stage_dev) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  e->stage_ptr = stage_dev;
  return KP1_OK;
}
int kp1_bind_population_stages(kp1_env* e, const kp1_curriculum_state* states_dev, int32_t n_replicas) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  if (!states_dev) {
    if (e->pop_states) e->pop_replicas = 0;   // (a bound dock population keeps its replica count)
    e->pop_states = nullptr;
    return KP1_OK;
  }
  if (e->pop_dock_states) return fail(KP1_ERR_UNSUPPORTED, "kp1_bind_population_stages: the handle is bound to a dock population");
  if (n_replicas < 1 || e->n % n_replicas != 0)
    return fail(KP1_ERR_INVALID, "kp1_bind_population_stages: the env count must be a multiple of the replica count");
  if (e->real_type != KP1_REAL_F32) return fail(KP1_ERR_UNSUPPORTED, "kp1_bind_population_stages: a population env handle is f32");
  if (e->cfg.env.mode != KP1_MODE_APPROACH || e->mode != KP1_MODE_APPROACH)
    return fail(KP1_ERR_UNSUPPORTED, "kp1_bind_population_stages: a population env handle runs the approach mode");
  e->pop_states = states_dev;
  e->pop_replicas = n_replicas;
  return KP1_OK;
}
int kp1_set_stream(kp1_env* e, void* stream) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  e->stream = (hipStream_t)stream;
  return KP1_OK;
}
int kp1_set_obs_stride(kp1_env* e, int32_t stride) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  if (stride != KP1_OBS_DIM && stride != 64) return fail(KP1_ERR_INVALID, "obs stride must be 56 or 64");
  e->obs_stride = stride;
  return KP1_OK;
}
int kp1_get_stage(const kp1_env* e, int32_t* stage_index) {
  if (!e || !stage_index) return fail(KP1_ERR_INVALID, "NULL argument");
  *stage_index = e->stage;
  return KP1_OK;
}
int kp1_set_mode(kp1_env* e, int32_t mode) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  if (mode != KP1_MODE_APPROACH && mode != KP1_MODE_DOCK) return fail(KP1_ERR_INVALID, "Unsupported policy mode");
  e->mode = mode;
  return KP1_OK;
}
int kp1_update_config(kp1_env* e, const kp1_config* cfg) {
  if (!e || !cfg) return fail(KP1_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  e->cfg.env = cfg->env;
  e->cfg.dock_reset = cfg->dock_reset;
  return upload_cfg(e);
}
int kp1_set_handoff_states(kp1_env* e, const kp1_handoff_state* states, int32_t n_states) {
  if (!e || (n_states > 0 && !states) || n_states < 0) return fail(KP1_ERR_INVALID, "bad handoff states");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  (void)hipFree(e->dev_handoff);
  e->dev_handoff = nullptr;
  e->n_handoff = n_states;
  if (n_states > 0) {
    HIP_TRY(hipMalloc((void**)&e->dev_handoff, sizeof(kp1_handoff_state) * (size_t)n_states));
    HIP_TRY(hipMemcpy(e->dev_handoff, states, sizeof(kp1_handoff_state) * (size_t)n_states, hipMemcpyHostToDevice));
  }
  return upload_cfg(e);
}
int kp1_set_route_stride_reset(kp1_env* e, const double* route_q, int32_t n_points, const int32_t* min_stride_by_stage, int32_t n_min,
                               const int32_t* max_stride_by_stage, int32_t n_max, const double* start_q_noise, const double* goal_q_noise,
                               double reverse_probability) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  HIP_TRY(hipSetDevice(e->device));
  if (!route_q || n_points == 0) {   // off: the Approach reset falls through to random-start pairs / the stage mixer again
    e->route_stride = kp1_env::RouteStride();
    return upload_cfg(e);
  }
  if (n_points < 2) return fail(KP1_ERR_INVALID, "kp1_set_route_stride_reset: a route needs at least two q waypoints");
  if (!min_stride_by_stage || !max_stride_by_stage || n_min < 1 || n_min > KP1_MAX_STAGES || n_max < 1 || n_max > KP1_MAX_STAGES)
    return fail(KP1_ERR_INVALID, "kp1_set_route_stride_reset: each stride list holds 1.." + std::to_string(KP1_MAX_STAGES) + " entries");
  if (!start_q_noise || !goal_q_noise) return fail(KP1_ERR_INVALID, "kp1_set_route_stride_reset: the two noise vectors are required");
  for (int k = 0; k < NJ; ++k)
    if (!(start_q_noise[k] >= 0.0) || !(goal_q_noise[k] >= 0.0)) return fail(KP1_ERR_INVALID, "kp1_set_route_stride_reset: a q noise is negative");
  if (!(reverse_probability == reverse_probability)) return fail(KP1_ERR_INVALID, "kp1_set_route_stride_reset: reverse_probability is NaN");
  // numpy's integers(lo, hi + 1) raises "low >= high" at the first reset of such a stage; here the table is refused before any kernel sees it
  for (int s = 0; s < KP1_MAX_STAGES; ++s) {
    const int lo = std::max(min_stride_by_stage[std::min(s, n_min - 1)], 1);
    if (lo > n_points - 1)
      return fail(KP1_ERR_INVALID, "kp1_set_route_stride_reset: stage " + std::to_string(s) + " needs a stride of at least " + std::to_string(lo) +
                                       ", the route of " + std::to_string(n_points) + " points allows " + std::to_string(n_points - 1));
  }
  kp1_env::RouteStride r;
  const size_t bytes = sizeof(double) * (size_t)n_points * NJ;
  HIP_TRY(hipMalloc((void**)&r.dev_q, bytes));
  e->route_tables.push_back(r.dev_q);
  HIP_TRY(hipMemcpyAsync(r.dev_q, route_q, bytes, hipMemcpyHostToDevice, e->stream));   // upload_cfg synchronizes the stream before it returns
  r.n_points = n_points;
  r.n_min = n_min;
  r.n_max = n_max;
  std::memcpy(r.min_stride, min_stride_by_stage, sizeof(int32_t) * (size_t)n_min);
  std::memcpy(r.max_stride, max_stride_by_stage, sizeof(int32_t) * (size_t)n_max);
  std::memcpy(r.start_noise, start_q_noise, sizeof r.start_noise);
  std::memcpy(r.goal_noise, goal_q_noise, sizeof r.goal_noise);
  r.reverse_probability = reverse_probability;
  e->route_stride = r;
  return upload_cfg(e);
}
int kp1_seed(kp1_env* e, uint64_t seed0, uint64_t first_env_id) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  HIP_TRY(hipSetDevice(e->device));
  return seed_streams(e, seed0, first_env_id);
}

int kp1_seed_blocks(kp1_env* e, const uint64_t* seeds, int32_t blocks, int32_t n_per_block) {
  if (!e || !seeds || blocks < 1 || n_per_block < 1 || (int64_t)blocks * n_per_block != e->n)
    return fail(KP1_ERR_INVALID, "kp1_seed_blocks: need blocks * n_per_block == N and one seed per block");
  HIP_TRY(hipSetDevice(e->device));
  const std::vector<uint64_t> sd(seeds, seeds + blocks);
  return seed_streams_by(e, [&](int64_t i) { return sd[(size_t)(i / n_per_block)] + (uint64_t)(i % n_per_block); });
}

int kp1_reset(kp1_env* e, const uint8_t* mask_dev, const kp1_reset_opts* opts, float* obs_dev) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  HIP_TRY(hipSetDevice(e->device));
  ResetOptsDev d = {nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  int mode = e->cfg.env.mode;  // reset() falls back to config.mode_name; arm_kinematic_env.py:111
  if (opts) {
    if (opts->policy_mode >= 0) {
      if (opts->policy_mode != KP1_MODE_APPROACH && opts->policy_mode != KP1_MODE_DOCK) return fail(KP1_ERR_INVALID, "Unsupported policy mode");
      mode = opts->policy_mode;
    }
    const double* const src[5] = {opts->initial_q, opts->initial_dq, opts->initial_prev_action, opts->goal_q, opts->goal_pose6};
    if (src[0] || src[1] || src[2] || src[3] || src[4]) {
      const double* dev[5];
      const int rc = upload_opt_rows(e, src, dev);
      if (rc != KP1_OK) return rc;
      const int flag[5] = {OPT_INITIAL_Q, OPT_INITIAL_DQ, OPT_INITIAL_PREV_ACTION, OPT_GOAL_Q, OPT_GOAL_POSE6};
      d = {dev[0], dev[1], dev[2], dev[3], dev[4], 0};
      for (int k = 0; k < 5; ++k)
        if (dev[k]) d.flags |= flag[k];
    }
  }
  e->mode = mode;
  return with_real(e->real_type, [&](auto real) { return launch_reset<decltype(real)>(e, mask_dev, d, mode, obs_dev); });
}

int kp1_step(kp1_env* e, const void* actions_dev, float* obs_dev, void* reward_dev, uint8_t* done_dev, float* terminal_obs_dev,
             int32_t auto_reset) {
  if (!e || !actions_dev || !obs_dev || !reward_dev || !done_dev) return fail(KP1_ERR_INVALID, "NULL buffer passed to kp1_step");
  HIP_TRY(hipSetDevice(e->device));
  return with_real(e->real_type, [&](auto real) { return launch_step<decltype(real)>(e, actions_dev, obs_dev, reward_dev, done_dev, terminal_obs_dev, auto_reset); });
}

int kp1_observe(kp1_env* e, float* obs_dev) {
  if (!e || !obs_dev) return fail(KP1_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  return with_real(e->real_type, [&](auto real) {
    using R = decltype(real);
    return launch_env(kp1_observe_kernel<R>, e->n, ENV_BLOCK, 0, e->stream, state_of<R>(e), (const DevCfg<R>*)e->dev_cfg, e->mode, obs_dev, e->obs_stride);
  });
}

int kp1_get_info(kp1_env* e, kp1_info_view* v) {
  if (!e || !v) return fail(KP1_ERR_INVALID, "NULL argument");
  const size_t rs = e->real_size(), n = (size_t)e->n;
  const char* base = (const char*)e->real;
  auto rf = [&](int f) { return (const void*)(base + rs * n * (size_t)f); };
  v->position_error_norm = rf(F_POS_ERR);
  v->orientation_error_norm = rf(F_ORI_ERR);
  v->min_position_error = rf(F_MIN_POS);
  v->executed_delta_q_l2 = rf(F_EXEC_DQ);
  v->action_l2 = rf(F_ACTION_L2);
  v->delta_q_change_l2 = rf(F_DQ_CHANGE);
  v->q = rf(F_Q);
  v->dq = rf(F_DQ);
  v->prev_action = rf(F_PREV_ACTION);
  v->goal_q = rf(F_GOAL_Q);
  v->goal_pose6 = rf(F_GOAL_POSE);
  v->ee_pose6 = rf(F_EE_POSE);
  v->entry_metrics = rf(F_ENTRY);
  v->episode_step = e->ints + n * I_STEP;
  v->dwell_count = e->ints + n * I_DWELL;
  v->near_goal_entry_count = e->ints + n * I_ENTRY;
  v->near_goal_drift_count = e->ints + n * I_DRIFT;
  v->flags = e->ints + n * I_FLAGS;
  v->stage_index = e->ints + n * I_STAGE;
  v->n_envs = e->n;
  v->real_type = e->real_type;
  return KP1_OK;
}

int kp1_eval_accumulate(kp1_env* e, const kp1_eval_buffers* b, const double* action_norm, const uint8_t* done, const uint8_t* active, int32_t step,
                        const double* ready_thresholds, int32_t handoff_confirm_steps, void* stream) {
  if (!e || !b || !b->metrics || !b->counters || !b->flags || !b->state || !b->n_alive) return fail(KP1_ERR_INVALID, "kp1_eval_accumulate: NULL buffer");
  if (step < 0 || (step > 0 && (!action_norm || !done))) return fail(KP1_ERR_INVALID, "kp1_eval_accumulate: a step needs action norms and done bytes");
  if (b->hand_metrics && (!b->hand_step || !b->hand_success || !b->hand_state)) return fail(KP1_ERR_INVALID, "kp1_eval_accumulate: incomplete handoff buffers");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t st = stream ? (hipStream_t)stream : e->stream;
  HIP_TRY(hipMemsetAsync(b->n_alive, 0, sizeof(int32_t), st));
  const bool track = ready_thresholds != nullptr;
  const double t0 = track ? ready_thresholds[0] : 0.0, t1 = track ? ready_thresholds[1] : 0.0, t2 = track ? ready_thresholds[2] : 0.0,
               t3 = track ? ready_thresholds[3] : 0.0;
  return with_real(e->real_type, [&](auto real) {
    using R = decltype(real);
    return launch_env(eval_accumulate_kernel<R>, e->n, UTIL_BLOCK, 0, st, (const R*)e->real, e->n, *b, action_norm, done, active, step, track, t0, t1, t2, t3,
                      handoff_confirm_steps);
  });
}

int kp1_enable_reward_components(kp1_env* e, int32_t enable) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  HIP_TRY(hipSetDevice(e->device));
  if (enable && !e->comps) {
    HIP_TRY(hipMalloc(&e->comps, e->real_size() * 64 * (size_t)e->n));
    HIP_TRY(hipMemsetAsync(e->comps, 0, e->real_size() * 64 * (size_t)e->n, e->stream));
  }
  e->comps_enabled = enable != 0;
  return KP1_OK;
}
int kp1_get_reward_components(kp1_env* e, const void** comps_dev, int32_t* n_components) {
  if (!e || !comps_dev || !n_components) return fail(KP1_ERR_INVALID, "NULL argument");
  if (!e->comps_enabled || !e->comps) return fail(KP1_ERR_INVALID, "reward components are not enabled");
  *comps_dev = e->comps;
  *n_components = kp1_num_components(e->mode);
  return KP1_OK;
}

static const char* const APPROACH_COMPONENT_NAMES[KP1_N_APPROACH_COMPONENTS] = {
    "position_progress", "global_orientation_progress", "near_field_orientation_progress", "orientation_progress",
    "orientation_milestone_bonus", "near_field_orientation_center", "pre_near_goal_bonus", "near_goal_bonus",
    "pre_near_to_near_progress", "near_goal_bonus_scale", "coarse_orientation_bonus", "handover_bonus",
    "handover_retention_bonus", "handover_dwell_bonus", "handover_leave_penalty", "handover_regression_penalty",
    "dock_coarse_ready_bonus", "dock_coarse_ready_retention_bonus", "dock_coarse_ready_dwell_bonus",
    "dock_coarse_ready_leave_penalty", "dock_coarse_ready_regression_penalty", "finisher_ready_bonus",
    "finisher_ready_retention_bonus", "finisher_ready_dwell_bonus", "finisher_ready_leave_penalty",
    "finisher_ready_regression_penalty", "near_handoff_action_penalty", "near_handoff_dq_penalty",
    "near_handoff_motion_bonus", "near_handoff_settle_bonus", "same_step_alignment_bonus", "dwell_bonus",
    "drift_penalty", "near_goal_leave_penalty", "drift_penalty_scale", "near_goal_entry_count", "near_goal_drift_count",
    "smoothness_penalty", "smoothness_multiplier", "joint_limit_penalty", "success_bonus", "curr_pos_error",
    "curr_ori_error", "curr_action_norm", "curr_dq_norm", "dwell_count", "in_pre_near_goal", "in_near_goal",
    "in_handover_zone", "in_dock_coarse_ready", "in_dock_coarse_ready_pose", "in_finisher_ready",
    "in_finisher_ready_pose", "in_near_handoff_zone"};
static const char* const DOCK_COMPONENT_NAMES[KP1_N_DOCK_COMPONENTS] = {
    "position_progress", "orientation_progress", "stay_in_zone_bonus", "dwell_bonus", "working_range_bonus",
    "working_range_dwell_bonus", "tight_pose_bonus", "tight_pose_dwell_bonus", "strict_pose_leave_penalty",
    "strict_center_reward", "strict_center_position_penalty", "strict_center_orientation_penalty",
    "strict_center_small_action_bonus", "strict_center_dwell_bonus", "tight_position_shaping",
    "tight_orientation_shaping", "convergence_position_progress", "convergence_orientation_progress",
    "orientation_position_gate_scale", "entry_action_penalty_scale", "leave_zone_penalty", "working_range_exit_penalty",
    "drift_penalty", "smoothness_penalty", "action_delta_violation_penalty", "delta_q_change_penalty",
    "preserve_state_bonus", "strict_hold_bonus", "low_motion_bonus", "tiny_correction_bonus", "worse_than_entry_penalty",
    "near_strict_regression_penalty", "aggressive_action_penalty", "dq_penalty", "joint_limit_penalty", "success_bonus",
    "basin_outer_bonus", "basin_inner_bonus", "basin_dwell_bonus", "basin_outer_exit_penalty", "basin_inner_exit_penalty",
    "basin_dwell_break_penalty", "basin_drift_penalty", "basin_zone_index", "curr_pos_error", "curr_ori_error",
    "dwell_count", "in_tight_pose", "in_near_strict", "entry_pos_error", "entry_ori_error", "entry_action_l2",
    "entry_dq_norm", "entry_to_curr_delta_position_error", "entry_to_curr_delta_orientation_error",
    "entry_to_curr_delta_action_l2", "entry_to_curr_delta_dq_norm", "near_goal_entry_count", "near_goal_drift_count",
    "in_near_goal"};
int kp1_num_components(int32_t mode) { return mode == KP1_MODE_DOCK ? KP1_N_DOCK_COMPONENTS : KP1_N_APPROACH_COMPONENTS; }
const char* kp1_component_name(int32_t mode, int32_t index) {
  if (index < 0 || index >= kp1_num_components(mode)) return "";
  return mode == KP1_MODE_DOCK ? DOCK_COMPONENT_NAMES[index] : APPROACH_COMPONENT_NAMES[index];
}

int kp1_get_state(kp1_env* e, double* q, double* dq, double* prev_action, double* goal_q, double* goal_pose6) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  HIP_TRY(hipSetDevice(e->device));
  OptScratch s;
  int rc = ensure_scratch(e, &s);
  if (rc == KP1_OK)
    rc = with_real(e->real_type, [&](auto real) {
      using R = decltype(real);
      return launch_env(kp1_get_state_kernel<R>, e->n, ENV_BLOCK, 0, e->stream, state_of<R>(e), s.dev[0], s.dev[1], s.dev[2], s.dev[3], s.dev[4]);
    });
  if (rc != KP1_OK) return rc;
  double* const dst[5] = {q, dq, prev_action, goal_q, goal_pose6};
  for (int k = 0; k < 5; ++k)
    if (dst[k]) HIP_TRY(hipMemcpyAsync(dst[k], s.dev[k], s.bytes[k], hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return KP1_OK;
}

int kp1_set_state(kp1_env* e, const double* q, const double* dq, const double* prev_action, const double* goal_q,
                  const double* goal_pose6, int32_t capture_entry_metrics) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  HIP_TRY(hipSetDevice(e->device));
  const double* const src[5] = {q, dq, prev_action, goal_q, goal_pose6};
  const double* dev[5];
  const int rc = upload_opt_rows(e, src, dev);
  if (rc != KP1_OK) return rc;
  return with_real(e->real_type, [&](auto real) {
    using R = decltype(real);
    return launch_env(kp1_set_state_kernel<R>, e->n, ENV_BLOCK, 0, e->stream, state_of<R>(e), (const DevCfg<R>*)e->dev_cfg, dev[0], dev[1], dev[2], dev[3], dev[4],
                      capture_entry_metrics);
  });
}

int kp1_rng_get(kp1_env* e, kp1_rng_state* out) {
  if (!e || !out) return fail(KP1_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  return download_rng_planes(e->rng64, e->rng32, out, (size_t)e->n, e->stream);
}
int kp1_rng_set(kp1_env* e, const kp1_rng_state* in) {
  if (!e || !in) return fail(KP1_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  return upload_rng_planes(e->rng64, e->rng32, in, (size_t)e->n, e->stream);
}

static int state_copy(kp1_env* e, bool save) {
  if (!e) return fail(KP1_ERR_INVALID, "env is NULL");
  HIP_TRY(hipSetDevice(e->device));
  const size_t n = (size_t)e->n;
  const size_t sizes[4] = {e->real_size() * F_NUM_REAL * n, sizeof(int32_t) * I_NUM_INT * n, sizeof(uint64_t) * 4 * n, sizeof(uint32_t) * 2 * n};
  void* live[4] = {e->real, e->ints, e->rng64, e->rng32};
  if (!e->snapshot) {
    if (!save) return fail(KP1_ERR_INVALID, "kp1_state_restore without a kp1_state_snapshot");
    HIP_TRY(hipMalloc(&e->snapshot, sizes[0] + sizes[1] + sizes[2] + sizes[3]));
  }
  char* shadow = (char*)e->snapshot;
  for (int k = 0; k < 4; ++k) {
    HIP_TRY(hipMemcpyAsync(save ? (void*)shadow : live[k], save ? live[k] : (const void*)shadow, sizes[k], hipMemcpyDeviceToDevice, e->stream));
    shadow += sizes[k];
  }
  return KP1_OK;
}
int kp1_state_snapshot(kp1_env* e) { return state_copy(e, true); }
int kp1_state_restore(kp1_env* e) { return state_copy(e, false); }

#ifdef KP1_ENV_TRACE
int kp1_debug_env_trace(unsigned long long* out, int clear) {
  HIP_TRY(hipDeviceSynchronize());
  if (out) HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(kp1_env_trace_buf), sizeof(unsigned long long) * KP1_ENV_TRACE_SLOTS * KP1_ENV_TRACE_WAVES));
  if (clear) {
    std::vector<unsigned long long> z(KP1_ENV_TRACE_SLOTS * KP1_ENV_TRACE_WAVES, 0ull);
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(kp1_env_trace_buf), z.data(), sizeof(unsigned long long) * z.size()));
  }
  return KP1_OK;
}
#endif

int kp1_fk_pose6(int32_t device, int32_t real_type, const void* q_dev, void* pose6_dev, int64_t n, void* stream) {
  if (!q_dev || !pose6_dev || n < 0) return fail(KP1_ERR_INVALID, "bad argument");
  if (n == 0) return KP1_OK;
  int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  DevFk<double> fk;   // the chain itself is fp64 for both real types; real_type is the type of q and pose6 in memory
  fold_fk<double>(&fk);
  struct DevBuf {   // freed on every return (hipFree waits for the kernel that reads it)
    void* p = nullptr;
    ~DevBuf() { (void)hipFree(p); }
  } dfk;
  HIP_TRY(hipMalloc(&dfk.p, sizeof fk));
  HIP_TRY(hipMemcpy(dfk.p, &fk, sizeof fk, hipMemcpyHostToDevice));
  rc = with_real(real_type, [&](auto real) {
    using R = decltype(real);
    return launch_env(kp1_fk_kernel<R>, n, UTIL_BLOCK, 0, (hipStream_t)stream, (const DevFk<double>*)dfk.p, (const R*)q_dev, (R*)pose6_dev, n);
  });
  if (rc != KP1_OK) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return KP1_OK;
}

int kp1_pose_error(int32_t device, int32_t real_type, const void* curr_dev, const void* goal_dev, void* pos_err_dev, void* ori_err_dev,
                   void* norms_dev, int64_t n, void* stream) {
  if (!curr_dev || !goal_dev || n < 0) return fail(KP1_ERR_INVALID, "bad argument to kp1_pose_error");
  if (n == 0) return KP1_OK;
  const int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  return with_real(real_type, [&](auto real) {
    using R = decltype(real);
    return launch_env(kp1_pose_error_kernel<R>, n, UTIL_BLOCK, 0, (hipStream_t)stream, (const R*)curr_dev, (const R*)goal_dev, (R*)pos_err_dev, (R*)ori_err_dev,
                      (R*)norms_dev, n);
  });
}

int kp1_joint_utils(int32_t device, int32_t real_type, const kp1_config* cfg, const void* q_dev, const void* dq_dev, void* clipped_dev,
                    void* margin_dev, void* q_norm_dev, void* dq_norm_dev, int64_t n, void* stream) {
  if (!cfg || (!q_dev && !dq_dev) || n < 0) return fail(KP1_ERR_INVALID, "bad argument to kp1_joint_utils");
  if (n == 0) return KP1_OK;
  const int rc = use_device(device);
  if (rc != KP1_OK) return rc;
  return with_real(real_type, [&](auto real) {
    using R = decltype(real);
    JointLimitsDev<R> lim;
    for (int k = 0; k < NJ; ++k) { lim.lower[k] = (R)cfg->joints.lower[k]; lim.upper[k] = (R)cfg->joints.upper[k]; lim.dlim[k] = (R)cfg->joints.delta_limit[k]; }
    return launch_env(kp1_joint_utils_kernel<R>, n, UTIL_BLOCK, 0, (hipStream_t)stream, lim, (const R*)q_dev, (const R*)dq_dev, (R*)clipped_dev, (R*)margin_dev,
                      (R*)q_norm_dev, (R*)dq_norm_dev, n);
  });
}

}  // extern "C"

#include "kp1_route.inc"
#include "kp1_dock_curriculum.inc"
