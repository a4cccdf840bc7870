/*
 * kp1_route.h -- C ABI of the route-curriculum environments of the MI355X kinematic_phase1 engine.
 *
 * Replaces, for N environments at once, the reference's
 *   kinematic_phase1/route/route_dataset.py:73-99          load_route_dataset   (FK per waypoint, path length, tangents, chunks)
 *   kinematic_phase1/route/route_reset_samplers.py:47-117  sample_route_reset
 *   kinematic_phase1/route/reward_route.py:36-143          route_ready, compute_route_reward
 *   kinematic_phase1/route/route_observation.py:31-61      augment_route_observation
 *   kinematic_phase1/route/route_env.py:29-212             RouteKinematicEnv          (sequence_enabled = 0)
 *   kinematic_phase1/route/route_sequence_env.py:29-278    RouteSequenceKinematicEnv  (sequence_enabled = 1)
 * Both wrappers drive an approach-mode base env (kp1.h) whose reward is discarded; a kp1_route handle borrows a kp1_env the
 * caller created with the route config's env block and owns the per-env route state and a second PCG64 stream per env
 * (the wrapper's own `self._rng`; env i is seeded default_rng(seed + first_env_id + i) like make_vec_env does).
 *
 * All pointers are HIP device pointers unless named *_host.  Returns KP1_OK or a negative kp1_status (kp1.h).
 */
#ifndef KP1_ROUTE_H
#define KP1_ROUTE_H

#include <stdint.h>

#include "kp1.h"

#ifdef __cplusplus
extern "C" {
#endif

/* reward_route.py:13-33 RouteRewardConfig, declaration order */
#define KP1_ROUTE_REWARD_FIELDS(X)                                                                                          \
  X(q_goal_progress_weight, 2.0) X(ee_position_progress_weight, 6.0) X(ee_orientation_progress_weight, 5.0)                 \
  X(route_tangent_progress_weight, 0.25) X(same_step_route_ready_bonus, 1.5) X(route_ready_dwell_bonus, 0.8)                \
  X(low_motion_near_waypoint_bonus, 0.4) X(orientation_regression_penalty_weight, 4.0) X(q_route_regression_penalty_weight, 1.0) \
  X(off_route_penalty_weight, 0.25) X(action_magnitude_weight, 0.02) X(action_delta_weight, 0.03) X(dq_penalty_weight, 0.8)   \
  X(no_progress_penalty, 0.02) X(route_ready_pos_threshold_m, 0.010) X(route_ready_ori_threshold_rad, 0.150)                 \
  X(route_ready_q_threshold, 0.080) X(route_ready_action_threshold, 0.25) X(route_ready_dq_threshold, 0.010)
typedef struct kp1_route_reward {
#define X(name, dflt) double name;
  KP1_ROUTE_REWARD_FIELDS(X)
#undef X
} kp1_route_reward;

/* route_reset_samplers.py:14-30 RouteResetSamplerConfig.  mode: 0 "mixed_prefix_segment" (or any other string: the drawn
 * mode stands), 1 prefix_start_reset, 2 random_prefix_reset, 3 segment_reset, 4 replay_reset, 5 recovery_reset */
typedef struct kp1_route_reset_cfg {
  int32_t mode, min_route_index, max_route_index, segment_start_index, segment_end_index, replay_start_index, replay_end_index, pad_;
  double prefix_start_reset_ratio, random_prefix_reset_ratio, segment_reset_ratio, replay_reset_ratio, recovery_reset_ratio;
  double q_noise_std, dq_noise_std, prev_action_noise_std;
} kp1_route_reset_cfg;

typedef struct kp1_route_config {
  kp1_route_reward reward;
  kp1_route_reset_cfg reset;
  int32_t include_route_keys;             /* route_observation.py RouteObservationConfig */
  int32_t sequence_enabled, sequence_length, reset_ready_streak_on_advance; /* route_sequence_env.py:20-26 */
} kp1_route_config;

/* drawn / explicit reset modes as reported in info["route_reset_mode"] */
enum { KP1_ROUTE_MODE_PREFIX_START = 0, KP1_ROUTE_MODE_RANDOM_PREFIX, KP1_ROUTE_MODE_SEGMENT, KP1_ROUTE_MODE_REPLAY, KP1_ROUTE_MODE_RECOVERY,
       KP1_ROUTE_MODE_EXPLICIT };

/* Observation with the route keys: the 17 Dict keys in SB3's sorted order -- the 56-float layout up to and including `q`, then
 * route_q_error 7, route_q_goal 7, route_scalar 3, route_tangent 7, then task_type 3, wp_ori_err 3, wp_pos_err 3. */
#define KP1_ROUTE_OBS_DIM 80
#define KP1_ROUTE_N_COMPONENTS 17  /* compute_route_reward's components dict, insertion order (reward_route.py:122-140) */

typedef struct kp1_route kp1_route;

/* route_q_host: [n_waypoints][7] f64 joint goals (the JSON's "route_q").  FK per waypoint runs on the device in fp64. */
int kp1_route_create(kp1_env* base_env, const kp1_route_config* cfg, const double* route_q_host, int32_t n_waypoints, uint64_t seed,
                     uint64_t first_env_id, kp1_route** out);
int kp1_route_destroy(kp1_route* r);
/* host copies of the dataset as load_route_dataset computes it: poses6 [W][6], route_progress_m [W], next_q_delta [W][7], chunk_id [W] */
int kp1_route_get_dataset(kp1_route* r, double* poses6_host, double* progress_host, double* next_q_delta_host, int32_t* chunk_id_host);
/* set_route_window (route_env.py:101-122): replaces reset.min/max_route_index */
int kp1_route_set_window(kp1_route* r, int32_t min_route_index, int32_t max_route_index);
int kp1_route_seed(kp1_route* r, uint64_t seed, uint64_t first_env_id);

/* ---- population handle: K replicas of N envs in one handle (block k = envs [k N, (k + 1) N)) -------------------------------------
 * base_env holds K * N envs.  Env i of replica k owns default_rng(seeds[k] + i) for both PCG64 streams, the base env's (re-seeded here with
 * kp1_seed_blocks) and the wrapper's: block k is bit for bit the handle kp1_route_create(seed = seeds[k], first_env_id = 0) makes on N envs.
 * Everything in the config is shared except the reset window: each replica has its own min / max route index, read by the resets of its
 * block.  kp1_route_set_window sets every window; a single handle is a population of one.  f32 base envs only. */
#define KP1_ROUTE_MAX_REPLICAS 16
int kp1_route_create_population(kp1_env* base_env, const kp1_route_config* cfg, const double* route_q_host, int32_t n_waypoints,
                                const uint64_t* seeds_host, int32_t replicas, kp1_route** out);
int kp1_route_num_replicas(const kp1_route* r);
/* set_route_window of replica k alone */
int kp1_route_set_replica_window(kp1_route* r, int32_t replica, int32_t min_route_index, int32_t max_route_index);

/* explicit reset (options{"route_index", "start_route_index", "initial_q", ...}); NULL members fall back as the wrappers do */
typedef struct kp1_route_reset_opts {
  const int32_t* route_index;       /* [N] or NULL = sample with the route stream */
  const int32_t* start_route_index; /* [N] or NULL = max(route_index - 1, 0) */
  const double* initial_q;          /* [N][7] (sequence env only) or NULL = waypoint(start).q_goal */
  const double* initial_dq;         /* [N][7] or NULL = 0 */
  const double* initial_prev_action;
  int32_t evaluator_state;          /* != 0: honour initial_q / initial_dq / initial_prev_action in the single-waypoint env too -- what
                                       eval_route_curriculum.py:62-83 does by resetting base_env and poking _route_index / _prev_info */
  int32_t pad_;
} kp1_route_reset_opts;
int kp1_route_reset(kp1_route* r, const uint8_t* mask, const kp1_route_reset_opts* opts, float* obs);
/* actions [N][7] (f32 or f64 like the base env); obs [N][obs_dim()]; reward [N]; done [N] KP1_DONE_* bits (SUCCESS = route /
 * sequence success); auto_reset != 0 resets finished envs in place after writing terminal_obs (may be NULL) */
int kp1_route_step(kp1_route* r, const void* actions, float* obs, void* reward, uint8_t* done, float* terminal_obs, int32_t auto_reset);
int kp1_route_obs_dim(const kp1_route* r);
/* row pitch of the observation buffers passed to reset / step (default obs_dim; the PPO loop uses the MFMA kernels' padded
 * widths 64 / 128 -- only the first obs_dim floats of a row are written) */
int kp1_route_set_obs_stride(kp1_route* r, int32_t stride);

typedef struct kp1_route_info_view {  /* device arrays [N], valid until the next call */
  const int32_t* route_index; const int32_t* start_route_index; const int32_t* last_route_index; const int32_t* reset_mode;
  const int32_t* ready_streak; const int32_t* completed_waypoints;
  const uint8_t* route_ready; const uint8_t* waypoint_success; const uint8_t* route_regression; const uint8_t* orientation_hit;
  const void* q_error_norm; const void* nearest_route_q_distance;  /* real type of the base env */
} kp1_route_info_view;
int kp1_route_get_info(kp1_route* r, kp1_route_info_view* out);
int kp1_route_enable_reward_components(kp1_route* r, int32_t enable);
int kp1_route_get_reward_components(kp1_route* r, const void** comps /* [17][N] */);
const char* kp1_route_component_name(int32_t index);
int kp1_route_rng_get(kp1_route* r, kp1_rng_state* out_host);
int kp1_route_rng_set(kp1_route* r, const kp1_rng_state* in_host);
void kp1_route_config_default(kp1_route_config* cfg);

/* ---- prefix curriculum on the device (route/route_curriculum.py:23-132, RoutePrefixCurriculumCallback) ----------------
 * The callback scans the finished episodes of every VecEnv step in env order, appends (success, route_ready, orientation hit, regression)
 * to four windows and promotes to the next prefix when the four window rates pass; promotion calls set_route_window(max = prefix, min = 1)
 * on all envs.  kp1_route_curriculum_observe does that scan on the device after each kp1_route_step (same stream): it reads the done
 * bytes the caller passes and the wrapper's own per-env flags, and on promotion rewrites the reset window in the device-resident route
 * config, so the rollout needs no host synchronisation and can be replayed from a hipGraph. */
#define KP1_ROUTE_CURRICULUM_MAX_STAGES 16
#define KP1_ROUTE_CURRICULUM_MAX_WINDOW 1024
#define KP1_ROUTE_CURRICULUM_MAX_HISTORY 32
typedef struct kp1_route_curriculum_event {
  int64_t total_timesteps;
  int32_t from_stage, to_stage, from_prefix_end_index, to_prefix_end_index;
  double recent_success_rate, recent_route_ready_hit_rate, recent_orientation_hit_rate, recent_regression_rate;
} kp1_route_curriculum_event;
typedef struct kp1_route_curriculum_state {
  int32_t stage_index, stage_episode_count, ring_len, ring_head;
  int32_t window_episodes, min_episodes_per_stage, n_stages, n_events;
  int32_t prefix_end_index[KP1_ROUTE_CURRICULUM_MAX_STAGES];
  int32_t ring_sums[4]; /* running sums of the four windows (the callback recomputes the means per finished episode) */
  double promotion_success_rate, promotion_route_ready_hit_rate, promotion_orientation_hit_rate, promotion_max_regression_rate;
  int64_t num_timesteps;
  uint8_t ring[4][KP1_ROUTE_CURRICULUM_MAX_WINDOW]; /* successes, ready_hits, orientation_hits, regressions */
  kp1_route_curriculum_event events[KP1_ROUTE_CURRICULUM_MAX_HISTORY];
} kp1_route_curriculum_state;

/* allocate the tracker in device memory and apply the first stage's window (_on_training_start) */
int kp1_route_curriculum_create(kp1_route* r, const int32_t* prefix_end_index, int32_t n_stages, double promotion_success_rate,
                                double promotion_route_ready_hit_rate, double promotion_orientation_hit_rate, double promotion_max_regression_rate,
                                int32_t window_episodes, int32_t min_episodes_per_stage, kp1_route_curriculum_state** out_dev);
int kp1_route_curriculum_destroy(kp1_route* r, kp1_route_curriculum_state* st_dev);
/* _on_step: dones[0..N) = the KP1_DONE_* bytes kp1_route_step just wrote; steps_per_call = env steps this call stands for */
int kp1_route_curriculum_observe(kp1_route* r, kp1_route_curriculum_state* st_dev, const uint8_t* dones, int32_t steps_per_call, void* stream);

/* ---- data parallel: per-step episode records and the chunked multi-rank tracker ----------------------------------------------
 * The tracker reads the wrapper's flag planes, which every kp1_route_step rewrites, so a chunk of steps cannot be replayed from them.
 * kp1_route_episode_records keeps one byte per env and step instead: bits 0-3 = the KP1_DONE_* bits of the step, then the wrapper's
 * flags of the same step.  It reads the planes on the device (capturable in a hipGraph, like the tracker). */
#define KP1_ROUTE_REC_READY       16
#define KP1_ROUTE_REC_ORI_HIT     32
#define KP1_ROUTE_REC_REGRESSION  64
int kp1_route_episode_records(kp1_route* r, const uint8_t* dones, uint8_t* records /* [N] */, void* stream);
/* records = the all-gathered [world][chunk_steps][n_local] bytes of kp1_route_episode_records (rank-major).  Replayed step by step and,
 * inside a step, rank by rank = global env id order: the (done, info) sequence RoutePrefixCurriculumCallback sees on ONE VecEnv of
 * world * n_local envs.  The clock advances by world * n_local per env step.  A promotion rewrites the reset window of THIS rank's device
 * route config; it takes effect for the resets of the next chunk. */
int kp1_route_curriculum_observe_chunk(kp1_route* r, kp1_route_curriculum_state* st_dev, const uint8_t* records, int32_t n_local,
                                       int32_t chunk_steps, int32_t world, void* stream);
/* copy the tracker to the host (synchronises the stream) and bring the host copy of the reset window up to date */
int kp1_route_curriculum_read(kp1_route* r, const kp1_route_curriculum_state* st_dev, kp1_route_curriculum_state* out_host, void* stream);

/* ---- population tracker: one kp1_route_curriculum_state per replica of a population handle ------------------------------------------
 * st_dev = K states back to back.  observe_population launches K workgroups: workgroup k scans the envs [k N, (k + 1) N) of the step in env
 * order, advances replica k's clock by steps_per_call and on promotion rewrites window k only -- replica k's tracker is the one a single
 * handle of N envs with seed seeds[k] would run.  The single-handle entry points (create / observe / observe_chunk) refuse a population
 * handle of K > 1: the data-parallel chunk tracker has no population form. */
int kp1_route_curriculum_create_population(kp1_route* r, const int32_t* prefix_end_index, int32_t n_stages, double promotion_success_rate,
                                           double promotion_route_ready_hit_rate, double promotion_orientation_hit_rate,
                                           double promotion_max_regression_rate, int32_t window_episodes, int32_t min_episodes_per_stage,
                                           kp1_route_curriculum_state** out_dev);
int kp1_route_curriculum_observe_population(kp1_route* r, kp1_route_curriculum_state* st_dev, const uint8_t* dones /* [K N] */,
                                            int32_t steps_per_call, void* stream);
/* replica k's tracker to the host (synchronises the stream); brings the host copy of window k up to date */
int kp1_route_curriculum_read_replica(kp1_route* r, const kp1_route_curriculum_state* st_dev, int32_t replica, kp1_route_curriculum_state* out_host,
                                      void* stream);

/* ---- chained sequential evaluation on the device (eval/eval_route_curriculum.py:57-248, evaluate_sequential_route) ---------------------------
 * The sequential evaluator runs waypoint after waypoint on one env: the episode of waypoint w + 1 starts from the final (q, dq, prev_action) of
 * waypoint w.  A chain does that for every row of a route handle at once, with the bookkeeping and the hand-over to the next waypoint in
 * kp1_route_chain_kernel after each route step, so R chains advance in lock step without a host read.  Rows are replica-major: R = K * C rows,
 * row r runs the chain start_index[r] .. end_index[r] (the caller feeds row r's observations to replica r / C's policy).
 * One kp1_route_chain_record per finished waypoint, float planes widened to double (exact).  min_q_error is the minimum over the episode's STEPS;
 * the evaluator's value also covers the episode's start state, whose joint error the host forms from start_q with the evaluator's own
 * np.linalg.norm call. */
typedef struct kp1_route_chain_record {
  int32_t route_index, success, route_ready_hit, max_ready_streak, first_ready_step /* -1 = none */, steps;
  double final_position_error, final_orientation_error, final_q_error, min_position_error, min_orientation_error, min_q_error;
  double final_action_magnitude, final_dq_norm;
  double final_q[7], final_dq[7], final_prev_action[7];
  double start_q[7];   /* q as the episode's reset left it (get_state after the reset), written when the episode opens */
} kp1_route_chain_record;
typedef struct kp1_route_chain kp1_route_chain;
/* start_index / end_index: host arrays [n_rows], 1 <= start <= end < n_waypoints; n_rows = the handle's env count.  stop_on_failure != 0: a row
 * ends at its first waypoint that does not succeed (the teacher recorder).  f32 handles without `sequence`, recorded reward components or an
 * attached prefix tracker. */
int kp1_route_chain_create(kp1_route* r, const int32_t* start_index_host, const int32_t* end_index_host, int32_t n_rows, int32_t stop_on_failure,
                           kp1_route_chain** out);
int kp1_route_chain_destroy(kp1_route* r, kp1_route_chain* chain);
/* every row -> waypoint start_index[row] from q = route_q[start - 1], dq = prev_action = 0, start_route_index 0, mode EXPLICIT (kp1_route_reset
 * with evaluator_state); obs [n_rows][stride] */
int kp1_route_chain_begin(kp1_route* r, kp1_route_chain* chain, float* obs);
/* kp1_route_step(auto_reset = 0) then kp1_route_chain_kernel, on the handle's stream.  tags: NULL or [n_rows][2] int32 = {route_index, step
 * inside the episode} of the step just taken, {-1, -1} for rows whose chain has ended.  A finished row keeps being stepped; nothing of it is read. */
int kp1_route_chain_step(kp1_route* r, kp1_route_chain* chain, const float* actions, float* obs, float* reward, uint8_t* done, int32_t* tags);
typedef struct kp1_route_chain_view {  /* device pointers, valid until kp1_route_chain_destroy */
  const kp1_route_chain_record* records;  /* [n_rows][max_len]; row r holds n_records[r] records, waypoints start_index[r] .. in order */
  const int32_t* n_records;               /* [n_rows] */
  const int32_t* n_alive;                 /* rows still running after the last kp1_route_chain_step */
  int32_t n_rows, max_len;
} kp1_route_chain_view;
int kp1_route_chain_get_view(kp1_route_chain* chain, kp1_route_chain_view* out);

/* ---- one-launch rollout step (kp1_ppo.h: kp1_mlp handles) -----------------------------------------------------------
 * kp1_mlp_forward(m, obs, ..., noise, ..., clipped_action, ...) followed by kp1_route_step(r, clipped_action, next_obs, reward, done,
 * terminal_obs, 1), bit for bit, as ONE kernel launch on `stream`: the policy workgroup of a 32-row tile samples the actions, steps the tile's
 * base envs, scans the route for the nearest waypoint and runs the route step with its auto-reset.
 * m: a K = 1 or a population handle at hidden 64 / 128 whose obs_dim is the route handle's (56 or 80); K = kp1_route_num_replicas(r); row i of
 * every buffer is env i of r (replica-major).  obs_stride: obs_dim or its padded width (64 / 128), and the stride set with
 * kp1_route_set_obs_stride (next_obs and terminal_obs have that pitch).  value, log_prob and terminal_obs may be NULL; noise is required.
 * Refused before any launch (status + kp1_last_error, outputs untouched): hidden 256, an fp64 base env, recorded route reward components, an
 * obs_dim / obs_stride / replica-count mismatch, an env count that is no multiple of K, n_waypoints > KP1_ROUTE_FUSED_MAX_WAYPOINTS,
 * next_obs == obs or any overlap of next_obs / terminal_obs with obs, different devices, NULL required arguments, a live kp1_route_chain. */
#define KP1_ROUTE_FUSED_MAX_WAYPOINTS 914   /* the joint table (n_waypoints x 7 floats) overlays the kernel's 32 x 68 + 32 x 132 float tiles */
struct kp1_mlp;
int kp1_mlp_forward_route_step(struct kp1_mlp* m, kp1_route* r, const float* obs, int32_t obs_stride, const float* noise, float* value,
                               float* action, float* log_prob, float* next_obs, float* reward, uint8_t* done, float* terminal_obs, void* stream);

/* ---- the chained evaluator's lock step in ONE launch (route_chain_step_kernel, hidden 64 / 128, fp32) ------------------------------------------
 * kp1_mlp_forward_route_chain_step = kp1_mlp_forward(m, obs, noise NULL, clipped -> action) + kp1_route_chain_step(r, chain, action, next_obs,
 * reward, done, tags), bit for bit for every row whose chain is alive.  The one difference: a row whose chain has ended is NOT stepped; it gets
 * its {-1, -1} tag and nothing else of it is written (env planes, next_obs / action / reward / done entries).  kp1_route_chain_run makes n_steps
 * such lock steps in one launch, in place on obs; a tile whose rows have all ended leaves early.  Both clear and then leave in the chain's
 * n_alive the rows still running after the last step, and launch on `stream`.
 * Refused before any launch (status + kp1_last_error, outputs untouched): NULL required arguments, hidden 256, what kp1_route_chain_step
 * refuses (an fp64 base env, a sequence handle, recorded reward components, an attached prefix tracker), an obs_dim / obs_stride / replica-count
 * mismatch (a single route handle of K C envs serves K replicas), a stride different from kp1_route_set_obs_stride, an env count that is no
 * multiple of K, n_waypoints > KP1_ROUTE_FUSED_MAX_WAYPOINTS, different devices, a chain of another handle or env count, next_obs overlapping
 * obs partially (next_obs == obs is the evaluator's normal use), n_steps outside [1, KP1_ROUTE_CHAIN_RUN_MAX_STEPS]. */
#define KP1_ROUTE_CHAIN_RUN_MAX_STEPS 1024   /* lock steps of one launch; the host splits longer chains into consecutive calls */

/* kp1_mlp_forward(m, obs, noise NULL, clipped -> action) + kp1_route_chain_step(r, chain, action, next_obs, reward, done, tags), ONE launch.
 * next_obs == obs (in place) or disjoint from obs; action and tags may be NULL. */
int kp1_mlp_forward_route_chain_step(struct kp1_mlp* m, kp1_route* r, kp1_route_chain* chain, const float* obs, int32_t obs_stride,
                                     float* action, float* next_obs, float* reward, uint8_t* done, int32_t* tags, void* stream);

/* n_steps lock steps in ONE launch, in place on obs; leaves in the chain's n_alive the rows still running after the last step */
int kp1_route_chain_run(struct kp1_mlp* m, kp1_route* r, kp1_route_chain* chain, float* obs, int32_t obs_stride,
                        float* reward, uint8_t* done, int32_t n_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KP1_ROUTE_H */
