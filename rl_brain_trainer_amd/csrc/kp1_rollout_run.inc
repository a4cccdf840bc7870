// kp1_rollout_run.inc -- ALL env steps of a PPO rollout span in one launch (kp1_rollout_run on an Hp = 128 handle, approach mode), and the
// critic of the whole span in a second, wide launch.  Included by kp1_mlp.hip inside its anonymous namespace as the last kernel file (uses
// RolloutStepArgs of kp1_rollout_step.inc, es_layer and the ES_* geometry, es_episode_env, head_dot, step_env_lane, store_obs_tile, and the
// statement files it shares with the other tile kernels: x tile, sampling tail, row re-read, tracker replay).  DESIGN.md sections 27, 28.
//
// rollout_run_kernel: grid = (row tiles of ES_BM rows, replicas), 256 threads, no z-plane.  A workgroup carries its ES_BM rows through steps
// t = 0 .. n_steps - 1; one iteration is plane 0 of rollout_step_kernel on slice t of every rollout buffer (the buffers are contiguous
// [T(+1)][K n][...] tensors: slice t lies t * K n rows behind slice 0), writing obs[t + 1], which the next iteration reads.
//   * Nothing crosses a tile: the policy is frozen, the noise was drawn before the launch, every env is stepped by one lane of one workgroup and
//     every output element has one writer.  No workgroup waits on another; the loop is bounded by n_steps.
//   * Observation hand-over: wave 0 stores the tile's rows of obs[t + 1] and all four waves load them as the next x tile.  Between the two
//     stands the __syncthreads at the bottom of the loop (workgroup scope is sufficient: one CU, one L1, written through -- the argument of
//     eval_step_kernel's episode form).
//   * The env index and the config address carry a run-time zero that the loop produces (the sign bit of a count that wave 0 leaves in LDS), as
//     in the episode evaluator: the ~100 state-plane addresses and the config reads stay inside the iteration instead of being lifted out of
//     the loop and spilled across the forward, and the reward arithmetic is contracted as in the step form.
//   * The critic does not feed the rollout: value[t] is read by the bootstrap and by GAE only.  rollout_value_kernel computes it for all steps
//     afterwards, blockIdx.z = t, with the code of rollout_step_kernel's plane 1.
// TRACK (the replica is one tile: n <= ES_BM): the workgroup that steps a replica's envs is also its PointCurriculum tracker.  After the env
// step wave 0 reads back the done bytes its lanes have just stored and lane 0 replays them by curriculum_kernel's rule (kp1_ppo.hip; only the
// serial branch of curriculum_scan can be reached below TRK_PARALLEL_MIN = 192 episodes, and it is shared: one text included by both,
// kp1_tracker_replay_body.inc, after num_timesteps += steps_per_call).  The scalar state lives in LDS across the span and is written back once at the end; the ring is updated in place in the tracker (lane 0 is its only
// reader and writer during the launch); stage_index is also stored at every promotion.  The env step takes its reset stage from the LDS copy
// (StepArgs::stage_index of the iteration, clipped as the bound-pointer form clips it), so no load of the stage can be lifted out of the loop
// and no cache stands between a promotion in step t and a reset in step t + 1.  Without TRACK a bound handle's stage does not move during the
// span (nothing observes), and step_env_lane reads it as rollout_step_kernel does.
// No float atomics anywhere.

struct RolloutRunArgs {
  RolloutStepArgs s;                   // slice 0 of every buffer: s.obs = obs[0] (read), s.env.obs = obs[1] (written); s.env.auto_reset = 1
  int64_t rows;                        // K n: rows per slice
  int n_steps;
  int steps_per_call;                  // TRACK: what one env step adds to every tracker's clock
  int track_stage;                     // TRACK: the handle's resets follow the trackers (bound, with curriculum stages)
  kp1_curriculum_state* trackers;      // TRACK: replica r's tracker at + r
};

constexpr int RR_TRK_STAGE = 0, RR_TRK_COUNT = 1, RR_TRK_LEN = 2, RR_TRK_HEAD = 3, RR_TRK_EVENTS = 4, RR_TRK_SUM = 5, RR_TRK_WORDS = 6;

// POP: step_env_lane's population form (per-replica stages read from the bound trackers); never together with TRACK, which hands the stage over itself
template <bool POP, bool TRACK>
__global__ void __launch_bounds__(ES_NTH) rollout_run_kernel(const RolloutRunArgs a) {
  static_assert(!(POP && TRACK), "the tracked form takes every replica's stage from its own LDS copy");
  __shared__ __attribute__((aligned(16))) float lds[ES_LDS_FLOATS];
  __shared__ int trk[TRACK ? RR_TRK_WORDS : 1];
  float* xs = lds;
  float* h1s = xs + ES_X_FLOATS;
  float* h2s = h1s + ES_H_FLOATS;
  float* acts = h2s + ES_H_FLOATS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned rep = blockIdx.y;
  const int m0 = blockIdx.x * ES_BM;
  const int64_t env0 = (int64_t)rep * a.s.n + m0;        // env of the tile's row 0
  const int rows_live = min(ES_BM, a.s.n - m0);
  const bool live = lane < rows_live;
  const int row = tid >> 3, out = tid & 7;
  const bool ok = m0 + row < a.s.n;
  const int stride = a.s.obs_stride;                     // the env handle's pitch too (the entry point checks)
  kp1_curriculum_state* st = nullptr;                    // no __restrict__: lane 0 reads ring entries it has stored
  long long timesteps = 0;                               // TRACK: lane 0 of wave 0

  if constexpr (TRACK) {
    st = a.trackers + rep;
    if (wave == 0) {
      // the window sum of the live entries (tracker_load of kp1_ppo.hip): the len positions from head on
      const int len = st->ring_len, head = st->ring_head, window = st->window_episodes;
      int part = 0;
      for (int k = lane; k < window; k += 64) {
        const int age = k >= head ? k - head : k - head + window;
        if (age < len) part += st->ring[k];
      }
      for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
      if (lane == 0) {
        trk[RR_TRK_STAGE] = st->stage_index; trk[RR_TRK_COUNT] = st->stage_episode_count; trk[RR_TRK_LEN] = len; trk[RR_TRK_HEAD] = head;
        trk[RR_TRK_EVENTS] = st->n_events; trk[RR_TRK_SUM] = part;
        timesteps = st->num_timesteps;
      }
    }
  }
  unsigned runtime_zero = 0;           // see es_episode_env

  for (int t = 0; t < a.n_steps; ++t) {
    const int64_t off = (int64_t)t * a.rows;             // slice t of a buffer starts `off` rows behind slice 0
    // ---- 1. the tile's rows of obs[t] -> LDS.  They are what wave 0 stored in the previous iteration: no __restrict__ on the pointer
    {
      constexpr int X_INP = ES_INP, X_PITCH = ES_XP;
      const int x_n = a.s.n, x_stride = stride, x_kreal = a.s.Kreal;
      const float* obs = a.s.obs + (off + (int64_t)rep * a.s.n) * stride;
#include "kp1_x_tile_body.inc"
    }
    __syncthreads();

    // ---- 2. hidden layers of the policy net
    es_layer<ES_INP>(xs, ES_XP, a.s.w1 + rep * a.s.r_w1, a.s.b1 + rep * a.s.r_b, h1s, wave, lane);
    __syncthreads();
    es_layer<ES_HP>(h1s, ES_HPITCH, a.s.w2 + rep * a.s.r_w2, a.s.b2 + rep * a.s.r_b, h2s, wave, lane);
    __syncthreads();

    // ---- 3. action heads and head_infer_kernel's sampling tail (rollout_step_kernel's, on slice t)
    {
      const float* __restrict__ w3 = a.s.w3 + rep * a.s.r_w3;
      const float* __restrict__ b3 = a.s.b3 + rep * a.s.r_b3;
      constexpr bool TAIL_STORES_CLIPPED = false;
      const RolloutStepArgs fw = a.s;  // a copy, not a reference: see the fragment's header
      const int64_t tail_off = off;
      float* const tail_clipped = nullptr;
#include "kp1_sample_tail_body.inc"
    }
    __syncthreads();

    // ---- 4. lane r of wave 0 steps env env0 + r (auto-reset included); then the wave stores the tile's rows of obs[t + 1]
    if (wave == 0) {
      StepArgs<float> env = es_episode_env(a.s.env, runtime_zero);
      env.reward = a.s.env.reward + off;
      env.done = a.s.env.done + off;
      env.terminal_obs = a.s.env.terminal_obs ? a.s.env.terminal_obs + off * stride : nullptr;
      if constexpr (TRACK) {
        if (a.track_stage) {
          env.stage_ptr = nullptr;
          env.stage_index = kp_clipi(trk[RR_TRK_STAGE], 0, kp_maxi(env.smp->n_stages - 1, 0));
        }
      }
      float o[KP1_OBS_DIM];
      if (live) {
        step_env_lane<float, KP1_MODE_APPROACH, false, POP>(env, env0 + lane + runtime_zero, acts + lane * 8, o);
      } else if (lane < ES_BM) {
        // A lane without an env fills `o` from a row of obs[t] (a valid one: clamped like the x tile's); store_obs_tile never stores it.
        // This is ES_EPISODE_REREADS of kp1_eval_step.inc, and as little a matter of taste: the env step's fp32 sums are not
        // contraction-pinned, and inside a loop the code around the inlined step decides how the compiler pairs and fuses them.  Without
        // this branch the sum of squares behind executed_delta_q_l2 comes out as fma(d1, d1, d0 d0) + d2 d2 + ... + d6 d6 where the step
        // form has d0 d0 + ... + d5 d5 followed by fma(d6, d6, .) (seen in the listings of both kernels, and as a last-bit difference of
        // that info plane on the GPU); with it the listing has the step form's chain in every instantiation.  tests/test_rollout_run_gpu.py
        // is the guard: after a compiler change that test says whether the choice still holds.
        const f32x4* src = reinterpret_cast<const f32x4*>(a.s.obs + (off + (int64_t)rep * a.s.n + min(m0 + lane, a.s.n - 1)) * stride);
#include "kp1_row_reread_body.inc"
      }
      // x and h1 were last read two barriers ago
      store_obs_tile(a.s.env.obs + off * stride, env0, rows_live, o, live, stride, lds);
      int n_done = 0;
      if constexpr (TRACK) {
        // the done byte this lane has just stored
        const unsigned d = live ? (unsigned)env.done[env0 + lane] : 0u;
        const bool ended = (d & (KP1_DONE_TERMINATED | KP1_DONE_TRUNCATED)) != 0u;
        unsigned long long m = __ballot(ended);
        const unsigned long long sm = __ballot(ended && (d & KP1_DONE_SUCCESS) != 0u);
        n_done = __popcll(m);
        if (lane == 0) {
          timesteps += a.steps_per_call;
          if (m) {
            int stage = trk[RR_TRK_STAGE], count = trk[RR_TRK_COUNT], len = trk[RR_TRK_LEN], head = trk[RR_TRK_HEAD];
            int n_events = trk[RR_TRK_EVENTS], sum = trk[RR_TRK_SUM];
            const int window = st->window_episodes, min_episodes = st->min_episodes_per_stage, max_stage = st->max_stage_index;
            const double threshold = st->success_rate_threshold;
            auto& ring = st->ring;                         // updated in place: lane 0 is its only reader and writer during the launch
            constexpr bool TRK_STORES_STAGE = true;        // the env steps that follow in this launch reset into the new stage
#include "kp1_tracker_replay_body.inc"
            trk[RR_TRK_STAGE] = stage; trk[RR_TRK_COUNT] = count; trk[RR_TRK_LEN] = len; trk[RR_TRK_HEAD] = head;
            trk[RR_TRK_EVENTS] = n_events; trk[RR_TRK_SUM] = sum;
          }
        }
      } else {
        n_done = rows_live;
      }
      if (lane == 0) reinterpret_cast<int*>(acts)[0] = n_done;   // acts: this wave alone read it, and has finished
    }
    __syncthreads();                   // the tile's rows of obs[t + 1] (and the tracker's stage), for the next iteration
    runtime_zero = (unsigned)__builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(acts)[0]) >> 31;   // a count is never negative
  }

  if constexpr (TRACK) {
    if (tid == 0) {
      st->stage_index = trk[RR_TRK_STAGE]; st->stage_episode_count = trk[RR_TRK_COUNT]; st->ring_len = trk[RR_TRK_LEN];
      st->ring_head = trk[RR_TRK_HEAD]; st->n_events = trk[RR_TRK_EVENTS]; st->num_timesteps = timesteps;
    }
  }
}

// value[t] of the whole span: plane 1 of rollout_step_kernel (x tile, the value net's two layers, head 7) on slice t = blockIdx.z.
// grid = (row tiles, replicas, n_steps).  Reads obs[0 .. n_steps), writes value; launched behind rollout_run_kernel on its stream.
__global__ void __launch_bounds__(ES_NTH) rollout_value_kernel(const RolloutRunArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[ES_LDS_FLOATS];
  float* xs = lds;
  float* h1s = xs + ES_X_FLOATS;
  float* h2s = h1s + ES_H_FLOATS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned rep = blockIdx.y;
  const int m0 = blockIdx.x * ES_BM;
  const int64_t off = (int64_t)blockIdx.z * a.rows;
  const int64_t env0 = (int64_t)rep * a.s.n + m0;
  {
    constexpr int X_INP = ES_INP, X_PITCH = ES_XP;
    const int x_n = a.s.n, x_stride = a.s.obs_stride, x_kreal = a.s.Kreal;
    const float* __restrict__ obs = a.s.obs + (off + (int64_t)rep * a.s.n) * a.s.obs_stride;
#include "kp1_x_tile_body.inc"
  }
  __syncthreads();
  es_layer<ES_INP>(xs, ES_XP, a.s.w1 + rep * a.s.r_w1 + a.s.n_w1, a.s.b1 + rep * a.s.r_b + a.s.n_b, h1s, wave, lane);
  __syncthreads();
  es_layer<ES_HP>(h1s, ES_HPITCH, a.s.w2 + rep * a.s.r_w2 + a.s.n_w2, a.s.b2 + rep * a.s.r_b + a.s.n_b, h2s, wave, lane);
  __syncthreads();
  const int row = tid >> 3, out = tid & 7;
  const float* __restrict__ w3 = a.s.w3 + rep * a.s.r_w3;
  const float* __restrict__ b3 = a.s.b3 + rep * a.s.r_b3;
  if (m0 + row < a.s.n && out == HEADS - 1) a.s.value[off + env0 + row] = head_dot(h2s + row * ES_HPITCH, w3 + out * ES_HP, ES_HP) + b3[out];
}
