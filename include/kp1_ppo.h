/*
 * kp1_ppo.h -- C ABI of the PPO-side device kernels of the MI355X kinematic_phase1 engine.
 *
 * The reference delegates PPO to stable_baselines3.PPO("MultiInputPolicy") (call sites:
 * kinematic_phase1/train_workspace_expansion.py:199,232; training/train_dock_policy.py:99,102).
 * SB3 2.8.0 (final_codes_docker/Dockerfile.demo:32) is absent from the reference tree and from this
 * image, so these kernels restate SB3's published semantics ("parity unpinned")
 * and are checked against plain PyTorch fp32 references of the same ops (tests/test_ppo_kernels_gpu.py).
 *
 * All pointers are HIP device pointers unless named *_host.  Layout [T][N] = time-major.
 * Every function returns KP1_OK or a negative kp1_status (kp1.h); text via kp1_last_error().
 */
#ifndef KP1_PPO_H
#define KP1_PPO_H

#include <stdint.h>

#include "kp1.h"

#ifdef __cplusplus
extern "C" {
#endif

/* RolloutBuffer.compute_returns_and_advantage (SB3 common/buffers.py): reverse GAE(lambda) scan, one lane per env.
 *   delta_t = r_t + gamma * V_{t+1} * (1 - done_t) - V_t ;  A_t = delta_t + gamma*lambda*(1 - done_t) * A_{t+1}
 *   V_T = last_values ; returns = A + V.   done_t = (done bits of step t) & (TERMINATED|TRUNCATED).
 * rewards/values/advantages/returns f32 [T][N]; dones u8 [T][N] (KP1_DONE_* bits as written by kp1_step). */
int kp1_gae_scan(int32_t device, const float* rewards, const float* values, const uint8_t* dones, const float* last_values,
                 float gamma, float gae_lambda, float* advantages, float* returns, int32_t T, int32_t N, void* stream);

/* kp1_gae_scan for a population whose replicas discount differently: N = K * n_per_replica columns, column i (replica i / n_per_replica)
 * uses gamma = gamma_lambda[2 r], lambda = gamma_lambda[2 r + 1] (device memory, f32 [K][2]) in kp1_gae_scan's expression order, so
 * column i equals a kp1_gae_scan of replica r's columns with those two scalars, bit for bit.  N % n_per_replica == 0. */
int kp1_gae_scan_replicas(int32_t device, const float* rewards, const float* values, const uint8_t* dones, const float* last_values,
                          const float* gamma_lambda, int32_t n_per_replica, float* advantages, float* returns, int32_t T, int32_t N, void* stream);

/* Time-limit bootstrap (SB3 on_policy_algorithm.collect_rollouts): rewards[t][i] += gamma * terminal_values[t][i]
 * where step t of env i was truncated and not terminated. */
int kp1_bootstrap_truncated(int32_t device, float* rewards, const float* terminal_values, const uint8_t* dones, float gamma,
                            int64_t count, void* stream);

/* Advantage statistics of every minibatch of an epoch in ONE launch (SB3 normalises per minibatch: ppo.py train(),
 * advantages = (adv - adv.mean()) / (adv.std() + 1e-8)).  Minibatch b = idx[b*minibatch .. min((b+1)*minibatch, total)) (idx NULL =
 * identity).  out_sums f64 [n_minibatches][3] = (sum, sum of squares, count): the host side (or, data parallel, ONE all-reduce per
 * epoch instead of one per minibatch) turns them into (mean, 1/(std+1e-8)) for kp1_mlp_loss_grad's adv_stats_dev. */
int kp1_adv_minibatch_sums(int32_t device, const float* advantages, const int64_t* idx, int64_t total, int64_t minibatch, double* out_sums,
                           void* stream);
/* Minibatch shuffle of one epoch (SB3 RolloutBuffer.get: indices = np.random.permutation(buffer_size * n_envs)): out[i] = P(i), i in [0, n),
 * with P a keyed pseudo-random permutation of [0, n) evaluated per element -- four rounds of (odd multiply + add, xorshift) modulo
 * 2^ceil(log2 n), each invertible, walked until the value lands below n (cycle walking; the index-shuffle construction of input
 * pipelines).  One elementwise launch instead of the radix sort + merge passes of a sort-based randperm (0.16 ms for 524288 elements,
 * eight times per PPO iteration).  keys: 8 x u32 (host memory) drawn by the caller per epoch; n <= 2^31. */
int kp1_random_permutation(int32_t device, int64_t n, const uint32_t* keys, int64_t* out, void* stream);

/* (sum, sum of squares, count) f64 [n_minibatches][3] (after the data-parallel all-reduce, if any) -> f32 [n_minibatches][2] =
 * (mean, 1 / (std + 1e-8)) with torch's unbiased std, in ONE launch (the same arithmetic in f64 as the tensor expressions it replaces:
 * thirteen elementwise launches per epoch inside the update graph). */
int kp1_adv_minibatch_stats(int32_t device, const double* sums, int64_t n_minibatches, float* out_stats, void* stream);

/* ---- device-resident PointCurriculumCallback (kinematic_phase1/training/callbacks.py:32-101) --------------------
 * The callback scans (done, info["success"]) in env order after every VecEnv step and may promote the stage for ALL
 * envs; resets inside that step already happened with the old stage.  Keeping the tracker on the device removes the
 * per-step host sync: kp1_curriculum_observe runs after each kp1_step on the same stream and publishes the stage in
 * device memory, from which the next kp1_step reads it (kp1_bind_stage_ptr). */
#define KP1_CURRICULUM_MAX_WINDOW 1024
#define KP1_CURRICULUM_MAX_HISTORY 64
typedef struct kp1_curriculum_event {
  int64_t total_timesteps; /* env steps taken (all ranks) when the promotion fired, like history["total_timesteps"] */
  int32_t from_stage, to_stage;
  double trigger_success_rate;
} kp1_curriculum_event;
typedef struct kp1_curriculum_state {
  int32_t stage_index;          /* current_stage_index; first word so an env kernel can read it as int32 */
  int32_t stage_episode_count;
  int32_t ring_len, ring_head;
  int32_t window_episodes, min_episodes_per_stage, max_stage_index, n_events;
  double success_rate_threshold;
  int64_t num_timesteps;
  int32_t ring[KP1_CURRICULUM_MAX_WINDOW];
  kp1_curriculum_event events[KP1_CURRICULUM_MAX_HISTORY];
} kp1_curriculum_state;

/* allocate + initialise a tracker in device memory (callbacks.py:33-51) */
int kp1_curriculum_create(int32_t device, double success_rate_threshold, int32_t window_episodes, int32_t min_episodes_per_stage,
                          int32_t max_stage_index, int32_t initial_stage_index, kp1_curriculum_state** out_dev);
int kp1_curriculum_destroy(int32_t device, kp1_curriculum_state* st_dev);
/* _on_step (callbacks.py:71-92): consume dones[0..n) (KP1_DONE_* bits) in index order; steps_per_call = env steps this
 * call represents (n_envs * world_size) for the num_timesteps clock. */
int kp1_curriculum_observe(int32_t device, kp1_curriculum_state* st_dev, const uint8_t* dones, int32_t n, int32_t steps_per_call, void* stream);
/* Data-parallel form: dones = the all-gathered [world][chunk_steps][n_local] done bytes of a chunk of env steps (rank-major).  Replayed
 * step by step and, inside a step, rank by rank = global env id order, i.e. exactly the (done, info) sequence the reference callback
 * would see on one VecEnv of world * n_local envs; the clock advances by world * n_local per env step.  A promotion takes effect for
 * the resets of the NEXT chunk (every rank runs this on identical bytes, so all ranks switch together). */
int kp1_curriculum_observe_chunk(int32_t device, kp1_curriculum_state* st_dev, const uint8_t* dones, int32_t n_local, int32_t chunk_steps,
                                 int32_t world, void* stream);
int kp1_curriculum_read(int32_t device, const kp1_curriculum_state* st_dev, kp1_curriculum_state* out_host, void* stream);
/* make kp1_step take its curriculum stage from *stage_dev (e.g. &tracker->stage_index) instead of kp1_set_stage */
int kp1_bind_stage_ptr(kp1_env* env, const int32_t* stage_dev);

/* Population of K trackers for a population env handle (block k = envs [k N, (k + 1) N) is replica k): K contiguous states, tracker k
 * starting on initial_stages[k] (host memory; clipped like kp1_curriculum_create's); the other settings are shared.  Free with
 * kp1_curriculum_destroy.  1 <= K <= KP1_CURRICULUM_MAX_REPLICAS. */
#define KP1_CURRICULUM_MAX_REPLICAS 16
int kp1_curriculum_create_population(int32_t device, int32_t n_replicas, double success_rate_threshold, int32_t window_episodes,
                                     int32_t min_episodes_per_stage, int32_t max_stage_index, const int32_t* initial_stages,
                                     kp1_curriculum_state** out_dev);
/* ONE launch of K one-wave workgroups: workgroup k replays dones[k N, (k + 1) N) into tracker k by kp1_curriculum_observe's rule (its
 * no-episode-ended early-out included); every clock advances by steps_per_call.  There is no data-parallel (chunk) form. */
int kp1_curriculum_observe_population(int32_t device, kp1_curriculum_state* states_dev, const uint8_t* dones, int32_t n_per_replica,
                                      int32_t n_replicas, int32_t steps_per_call, void* stream);
/* kp1_curriculum_read of tracker k of a population of n_replicas */
int kp1_curriculum_read_replica(int32_t device, const kp1_curriculum_state* states_dev, int32_t n_replicas, int32_t k,
                                kp1_curriculum_state* out_host, void* stream);
/* Population env handle: from now on env i of kp1_step's auto-reset takes its stage from states_dev[i / (N / n_replicas)].stage_index
 * (one launch of the population form of the step kernel for all K replicas); kp1_reset keeps the handle's host stage.  Needs
 * N % n_replicas == 0, the approach mode and the f32 handle; the fused policy + env step refuses a bound handle.  states_dev NULL unbinds. */
int kp1_bind_population_stages(kp1_env* env, const kp1_curriculum_state* states_dev, int32_t n_replicas);

/* ---- device-resident DockReverseCurriculumCallback (kinematic_phase1/training/callbacks.py:104-212) -------------
 * The Finisher's reverse curriculum: after every VecEnv step the callback scans (done, info["success"]) in env order, keeps the last
 * `window_episodes` success bits and, when the current stage has seen `min_episodes` episodes and the newest `stage window` of them reach
 * `success_rate_threshold`, applies the next stage's overrides to all envs (apply_dock_training_stage, arm_kinematic_env.py:459-487).
 * A stage here carries the RESOLVED values (base config overlaid by the payloads of stages 0..k in order, which is what the env holds after
 * k promotions); the tracker writes them into the device config the step / reset kernels read. */
#define KP1_DOCK_CURRICULUM_MAX_STAGES 16
#define KP1_DOCK_CURRICULUM_MAX_WINDOW 1024
#define KP1_DOCK_CURRICULUM_MAX_HISTORY 32
typedef struct kp1_dock_curriculum_stage {
  double action_delta_scale, dock_residual_action_limit, dock_delta_q_change_limit_scale;             /* env scalars */
  double close_bucket_probability, close_bucket_min_pos_error_m, close_bucket_max_pos_error_m, close_bucket_max_ori_error_rad,
         handoff_state_probability;                                                                    /* dock_reset scalars */
  double close_init_q_noise[KP1_NJ], init_q_noise[KP1_NJ];
  double success_rate_threshold;     /* stage.get("success_rate_threshold", 1.0) */
  int32_t min_episodes;              /* stage.get("min_episodes", window_episodes) */
  int32_t window_episodes;           /* stage.get("window_episodes", window_episodes) */
  /* handoff-state buffer of this stage (stages may override handoff_state_buffer_path and the three handoff_state_max_* filters,
   * reset_samplers.py:131-165): a slice [offset, offset + count) of the buffer given to kp1_set_handoff_states, which then holds the
   * filtered lists of all stages back to back.  count < 0: the stage does not manage the buffer (the env's whole buffer stays in use). */
  int32_t handoff_offset, handoff_count;
} kp1_dock_curriculum_stage;
typedef struct kp1_dock_curriculum_event {
  int64_t total_timesteps;
  int32_t from_stage, to_stage, stage_episode_count, reserved0;
  double trigger_success_rate;
} kp1_dock_curriculum_event;
typedef struct kp1_dock_curriculum_state {
  int32_t stage_index, stage_episode_count, ring_len, ring_head, window_episodes, n_stages, n_events, reserved0;
  int64_t num_timesteps;
  kp1_dock_curriculum_stage stages[KP1_DOCK_CURRICULUM_MAX_STAGES];
  kp1_dock_curriculum_event events[KP1_DOCK_CURRICULUM_MAX_HISTORY];
  uint8_t ring[KP1_DOCK_CURRICULUM_MAX_WINDOW];
} kp1_dock_curriculum_state;
/* allocate the tracker next to a dock-mode env and apply stage 0 (_on_training_start) */
int kp1_dock_curriculum_create(kp1_env* env, const kp1_dock_curriculum_stage* stages_host, int32_t n_stages, int32_t window_episodes,
                               kp1_dock_curriculum_state** out_dev);
int kp1_dock_curriculum_destroy(kp1_env* env, kp1_dock_curriculum_state* st_dev);
/* _on_step: dones = [world][chunk_steps][n_local] done bytes (one process, one env step: world = chunk_steps = 1), replayed step by step
 * and rank by rank = global env order; the clock advances by world * n_local per env step */
int kp1_dock_curriculum_observe(kp1_env* env, kp1_dock_curriculum_state* st_dev, const uint8_t* dones, int32_t n_local, int32_t chunk_steps, int32_t world,
                                void* stream);
/* copy the tracker to the host; also brings the env handle's host-side config mirror in step with the stage the device applied */
int kp1_dock_curriculum_read(kp1_env* env, const kp1_dock_curriculum_state* st_dev, kp1_dock_curriculum_state* out_host, void* stream);
/* Dock population: K trackers for a dock-mode population env handle (block k = envs [k N, (k + 1) N) is replica k), each set up as
 * kp1_dock_curriculum_create sets one up, followed in the same allocation by K live stage records (record k = the stage tracker k is on,
 * stage 0 to begin with).  Applies stage 0 to the shared config before the first reset and binds the handle: kp1_step and kp1_reset then run
 * their dock population forms, env i reading what a stage overrides from live record i / N.  Needs the dock mode, the f32 handle,
 * N % n_replicas == 0, 1 <= n_replicas <= KP1_CURRICULUM_MAX_REPLICAS, a handle bound to no population and carrying no single dock tracker;
 * the fused policy + env step refuses a bound handle.  Free (and unbind) with kp1_dock_curriculum_destroy. */
int kp1_dock_curriculum_create_population(kp1_env* env, const kp1_dock_curriculum_stage* stages_host, int32_t n_stages, int32_t window_episodes,
                                          int32_t n_replicas, kp1_dock_curriculum_state** out_dev);
/* ONE launch of K one-wave workgroups: workgroup k replays dones[k N, (k + 1) N) into tracker k by kp1_dock_curriculum_observe's rule, its
 * clock advancing by N; a promotion rewrites only tracker k and live record k (never the shared config) */
int kp1_dock_curriculum_observe_population(kp1_env* env, kp1_dock_curriculum_state* states_dev, const uint8_t* dones, int32_t n_per_replica,
                                           int32_t n_replicas, void* stream);
/* copy tracker k of a population of n_replicas to the host; the handle's shared host config mirror is left as it is */
int kp1_dock_curriculum_read_replica(kp1_env* env, const kp1_dock_curriculum_state* states_dev, int32_t n_replicas, int32_t k,
                                     kp1_dock_curriculum_state* out_host, void* stream);

/* ---- actor-critic MLP on the matrix cores (fp32-in / fp32-accumulate MFMA, exact f32) ---------------------------
 * SB3 MultiInputActorCriticPolicy with net_arch pi = vf = [H, H], tanh:
 *   h1 = tanh(x W1^T + b1); h2 = tanh(h1 W2^T + b2); mean = h2p Wa^T + ba (7); value = h2v Wv^T + bv (1).
 * Both nets (index 0 = policy, 1 = value) run in one launch (grid.z).  H must be a multiple of 128 or equal to 64.
 * Kernel-format weights ("kw", see kp1_mlp_pack_weights) hold W1 zero-padded to 64 input columns, W2 and W2^T. */
#define KP1_MLP_IN 56
#define KP1_MLP_IN_PAD 64
#define KP1_MLP_IN_ROUTE 80      /* with the route observation keys (route/route_observation.py:14-61); padded to 128 */
#define KP1_MLP_IN_ROUTE_PAD 128
#define KP1_MLP_ACT 7

typedef struct kp1_mlp kp1_mlp; /* workspace: packed weights, activations, gradients for up to max_batch rows */

int kp1_mlp_create(int32_t device, int32_t hidden, int32_t max_batch, kp1_mlp** out);
/* same, for an observation of obs_dim floats: 56 (ArmKinematicEnv, observation_builder.py:29-94) or 80 (the route wrappers with
 * include_route_keys, route/route_env.py:186-207).  Rows are read with pitch obs_dim or the padded width (64 / 128). */
int kp1_mlp_create_ex(int32_t device, int32_t hidden, int32_t obs_dim, int32_t max_batch, kp1_mlp** out);
/* Population handle: K = `replicas` (1..KP1_MLP_MAX_REPLICAS) independent copies of the net -- K weight packs, activation workspaces and
 * gradient partials -- trained through ONE launch sequence with the replica on a grid axis (z = 2 * replica + net, or grid.y).  hidden 64 or
 * 128 (the layer-wise Hp = 128 kernels); obs_dim 56 (padded to 64) or 80 (the route observation, padded to 128: layer 1 and dW1 then run
 * over 128 input columns per replica).  Each replica computes exactly what a K = 1 handle computes on the same
 * inputs: reductions keep a single handle's order and chunking per replica, under KP1_MLP_OPT_TRAIN_TILE too (its chunking is a function of
 * n alone).  kp1_mlp_create / _create_ex make K = 1 handles.
 * Buffer layout of the entry points below for a K-replica handle (K = 1: the layouts documented at each entry point):
 *   kp1_mlp_pack_weights, kp1_mlp_adam_step: params, grad, exp_avg, exp_avg_sq are [K][num_params]; one clip norm per replica, one shared
 *     Adam step count (all replicas step together) unless a KL gate is set (kp1_mlp_set_kl_gate: one count per replica);
 *   kp1_mlp_forward: obs holds K * n rows, replica-major (replica r = rows [r n, (r + 1) n)); n = rows per replica; every output likewise
 *     [K][n][...];
 *   kp1_mlp_loss_grad: idx (required) is int64 [K][n], row indices into the shared obs / actions / old_log_prob / advantages / returns
 *     buffers; grad_out [K][num_params]; stats_out [K][4]; adv_stats_dev [K][2] (mean, 1/(std + 1e-8) of each replica's minibatch);
 *   kp1_mlp_forward_env_step: the layer-wise form below, replica k owning rows [k n, (k + 1) n) of every buffer;
 *   kp1_mlp_time_kernels and the KP1_MLP_OPT_BF16X3_WGRAD option return KP1_ERR_UNSUPPORTED. */
#define KP1_MLP_MAX_REPLICAS 16
int kp1_mlp_create_population(int32_t device, int32_t hidden, int32_t obs_dim, int32_t max_batch, int32_t replicas, kp1_mlp** out);
/* K of the handle (1 for kp1_mlp_create / _create_ex), 0 for NULL */
int32_t kp1_mlp_replicas(const kp1_mlp* m);
/* Per-replica PPO hyper-parameters of a population handle (a hyper-parameter sweep in one launch sequence).  The handle owns a device copy
 * of `host` [n]; n must equal K, n = 0 clears it, a K = 1 handle refuses a table.  While a table is set, replica k's kernels read entry k
 * (once per workgroup, at kernel entry) in place of the scalar arguments: kp1_mlp_loss_grad's clip_range, vf_coef and ent_coef,
 * kp1_mlp_adam_step's lr, eps and max_grad_norm.  Only the operand source changes: replica k with entry h computes bit for bit what a
 * K = 1 handle computes when called with h's scalars.  The table lives in device memory, so a captured graph holds only its address and
 * sees a later kp1_mlp_set_replica_hparams; setting or clearing it after a capture changes which source a re-capture uses.  Copies in
 * stream order and waits for the copy; not while `stream` is being captured. */
typedef struct kp1_replica_hparams {
  float learning_rate, adam_eps, max_grad_norm, clip_range, ent_coef, vf_coef;
} kp1_replica_hparams;
int kp1_mlp_set_replica_hparams(kp1_mlp* m, const kp1_replica_hparams* host, int32_t n, void* stream);
/* The same table written by ONE small launch, for every handle, K = 1 included: n must equal K; the K entries travel
 * as kernel arguments and the launch writes the handle's table with plain vector stores.  No copy from caller memory is queued and nothing
 * waits for `stream`: `host` is free on return.  Stream ordered -- launches already queued read the old values, later ones the new -- and
 * capturable (the captured values are then the baked ones; call it eagerly to change what a captured graph reads).  From the first
 * successful call on, replica k's kernels read entry k in place of the scalar arguments, exactly as after kp1_mlp_set_replica_hparams, and
 * a K = 1 handle does so too: it launches the table-reading forms of those kernels for its one replica (hidden 256: mlp_tile_line_kernel
 * and head_train_kernel<256, true>), bit for bit what the scalar forms compute on the same values.  kp1_mlp_set_replica_hparams(m, NULL, 0,
 * ...) returns any handle to its scalar arguments.  Refused before anything is written: NULL arguments, n != K, a non-finite field, and a
 * K = 1 handle with KP1_MLP_OPT_BF16X3_WGRAD on (KP1_ERR_UNSUPPORTED: the experiment has no line form; the option is likewise refused
 * while a line is on).  While a K = 1 handle reads its line kp1_mlp_anchor_loss_grad / kp1_mlp_anchor_adam_step return
 * KP1_ERR_UNSUPPORTED (their K = 1 forms take scalars). */
int kp1_mlp_hparams_store(kp1_mlp* m, const kp1_replica_hparams* host, int32_t n, void* stream);
int kp1_mlp_destroy(kp1_mlp* m);
/* number of f32 parameters in SB3 state_dict order (log_std, pi.0.w, pi.0.b, pi.2.w, pi.2.b, vf.0.w, ..., action_net.w/b, value_net.w/b) */
int64_t kp1_mlp_num_params(int32_t hidden);
int64_t kp1_mlp_num_params_ex(int32_t hidden, int32_t obs_dim);
/* repack the flat SB3-order parameter vector into kernel-format weights (call after every optimiser step) */
int kp1_mlp_pack_weights(kp1_mlp* m, const float* params, void* stream);

/* policy.forward for a rollout step: obs f32 [n][obs_stride] (first 56 columns used; obs_stride 56 or 64 with zero pad),
 * noise f32 [n][7] ~ N(0,1) or NULL (deterministic).  Outputs (any may be NULL):
 *   mean[n][7], value[n], action[n][7] = mean + exp(log_std) * noise, clipped_action[n][7] = clip(action, -1, 1),
 *   log_prob[n] = sum_d N(action_d; mean_d, std_d). */
int kp1_mlp_forward(kp1_mlp* m, const float* obs, int32_t obs_stride, int32_t n, const float* noise, float* mean, float* value,
                    float* action, float* clipped_action, float* log_prob, void* stream);

/* One rollout step in ONE launch: policy.forward on the current observations of ALL envs of `env` (row m = env m; obs f32 [N][obs_stride]),
 * Gaussian sampling, then VecEnv.step(clip(action)) of every env with the auto-reset -- SB3's collect_rollouts body
 * (on_policy_algorithm.py: policy(obs) -> clip -> env.step) without the action round trip through HBM and without a launch for the env.
 * Same results, bit for bit, as kp1_mlp_forward followed by kp1_step (tests/test_ppo_kernels_gpu.py, tests/test_rollout_step_layerwise_gpu.py).
 * fp32 env handles in approach or dock mode, 56-float observations (obs_stride 56 or 64); reward components must be off.  value / log_prob may
 * be NULL (value NULL skips the value net); terminal_obs may be NULL.
 *   hidden 256       a K = 1 handle with the tile path on (the rollout form of the 2x256 inference tile); env handles with bound population
 *                    stages or dock stage records are refused.
 *   hidden 64 / 128  a K = 1 or a population handle (rollout_step_kernel: grid = row tiles x K x {policy net + env step, value net}).  The env
 *                    handle holds K * n envs, row m of replica k being env k n + m; noise and every output are replica-major.  A handle with
 *                    bound population stages (kp1_bind_population_stages) or dock stage records (kp1_dock_curriculum_create_population) is
 *                    accepted when its replica count is K: env i then resets / steps on the stage of replica i / n, as kp1_step does.  On an
 *                    unbound handle the replicas share the host stage.  noise is required, and next_obs and terminal_obs must not overlap obs anywhere
 *                    (the value net's workgroups read rows that the policy net's workgroups would overwrite).
 * Refused before any launch: the 80-float route observation, f64 env handles, recorded reward components, modes other than approach and
 * dock, a replica-count mismatch, an env count that is no multiple of K, next_obs == obs or any overlap of next_obs / terminal_obs with obs (layer-wise form), different devices, NULL required
 * arguments, obs_stride other than 56 or 64.  (A kp1_route handle is not a kp1_env and has no step of its own here: its
 * one-launch rollout step is kp1_mlp_forward_route_step, include/kp1_route.h.) */
int kp1_mlp_forward_env_step(kp1_mlp* m, kp1_env* env, const float* obs, int32_t obs_stride, const float* noise, float* value, float* action,
                             float* log_prob, float* next_obs, float* reward, uint8_t* done, float* terminal_obs, void* stream);

/* ALL env steps of a rollout span in one launch (hidden 64 / 128, approach mode): n_steps times what
 * kp1_mlp_forward_env_step (and, with `trackers`, kp1_curriculum_observe / kp1_curriculum_observe_population after it) does per step, bit for
 * bit -- every buffer, the env handle and the trackers.  A workgroup carries its 32 rows through all steps; value[t] of the whole span is
 * computed by a second, wide launch behind it, and only if `value` is given.
 *   Every buffer is the contiguous rollout buffer from the slice of the span's first step on, a slice being the K n rows of one step
 * (replica-major, as kp1_mlp_forward_env_step takes them): obs holds n_steps + 1 slices at pitch obs_stride, slice t + 1 being step t's
 * next_obs; noise [n_steps][K n][7], action likewise, value / log_prob / reward / done [n_steps][K n], terminal_obs [n_steps][K n][obs_stride].
 * value, log_prob and terminal_obs may be NULL.  Two consecutive calls over [0, a) and [a, T) (the second on the buffers from slice a on) leave
 * everything exactly as one call over [0, T).
 *   trackers: NULL, or the tracker(s) the env handle's resets are bound to -- one state for K = 1 (bound with kp1_bind_stage_ptr to its
 * stage_index), the K contiguous states of a population (kp1_bind_population_stages).  The workgroup that steps a replica's envs then replays
 * each step's done bytes into the replica's tracker by kp1_curriculum_observe's rule, every clock advancing by steps_per_call per env step,
 * and a promotion in step t moves the resets of step t + 1.  This needs a replica to be one row tile: at most 32 envs per replica.  With
 * trackers == NULL a bound handle is accepted and its stage does not move during the span (nothing observes).
 *   Refused before any launch, outputs untouched: hidden 256, the 80-float observation, f64 handles, recorded reward components, the dock
 * mode and handles bound to dock stage records, a replica-count mismatch, an env count that is no multiple of K, obs_stride other than 56 or
 * 64 or than the env handle's pitch, NULL required arguments (noise included), n_steps < 1 or above KP1_ROLLOUT_RUN_MAX_STEPS, terminal_obs
 * overlapping the obs buffer, different devices, trackers that are not the handle's bound stage source, trackers with more than 32 envs per
 * replica, trackers with a negative steps_per_call. */
#define KP1_ROLLOUT_RUN_MAX_STEPS 2048   /* the longest n_steps of a committed config; the host splits a longer rollout */
int kp1_rollout_run(kp1_mlp* m, kp1_env* env, float* obs, int32_t obs_stride, const float* noise, float* value, float* action,
                    float* log_prob, float* reward, uint8_t* done, float* terminal_obs, int32_t n_steps,
                    kp1_curriculum_state* trackers, int32_t steps_per_call, void* stream);

/* One step of the batched deterministic evaluator (kp1_eval_accumulate's episodes) in ONE launch: the deterministic policy of `m` on the
 * current observations of ALL envs of `env`, action = clip(mean, -1, 1), its fp64 norm sqrt(a0^2 + ... + a6^2) (products and sums in index
 * order, uncontracted), the env step without auto-reset, and kp1_eval_accumulate's bookkeeping of env step number `step` for every buffer
 * of `buffers`, n_alive included.  Same results, bit for bit, as kp1_mlp_forward (noise NULL, clipped_action) + that norm + kp1_step
 * (auto_reset 0) + kp1_eval_accumulate (tests/test_population_eval_gpu.py, tests/test_eval_step_h256_gpu.py).
 *   m         56-float observations.  Hidden 64 or 128: a K = 1 or a population handle (eval_step_kernel).  Hidden 256: a K = 1 handle
 *             with the tile path on (the default; KP1_ERR_UNSUPPORTED after it was switched to the layer-wise kernels), which runs the
 *             evaluation form of the 2x256 inference tile.  Only the policy net runs, no activation workspace is used (max_batch does not
 *             bound the env count)
 *   env       fp32 handle of K * n envs in approach or dock mode, reward components off, no bound tracker / population stages;
 *             row m of replica k is env k n + m
 *   obs       f32 [K n][the handle's obs stride, 56 or 64]: read (this step's observations) and overwritten (the next step's); a workgroup
 *             reads its own rows before it writes them.  reward f32 [K n] and done u8 [K n] are written as kp1_step writes them.  These
 *             are the buffers kp1_reset / kp1_step take: the handle itself owns none
 *   step      >= 1; step 0 (initialisation after a reset, with the `active` mask) stays with kp1_eval_accumulate
 *   stream    the launch stream (NULL: the default stream)
 * Everything it cannot run is refused with a status and kp1_last_error text before any launch. */
int kp1_eval_step(kp1_mlp* m, kp1_env* env, float* obs, float* reward, uint8_t* done, const kp1_eval_buffers* buffers, int32_t step,
                  const double* ready_thresholds /* [4] or NULL */, int32_t confirm_steps, void* stream);

/* Env steps first_step .. last_step of the same evaluator in ONE launch: a workgroup carries its 32 rows through all of them by itself and
 * leaves when its last episode has ended (nothing crosses a row tile in the evaluator, so workgroups never wait for each other).  Same
 * handles, arguments and refusals as kp1_eval_step, plus: first_step < 1, last_step < first_step, and a span of more than
 * KP1_EVAL_EPISODES_MAX_STEPS steps (the bound of one launch; the host splits a longer limit into consecutive calls).  Everything is
 * refused before any launch.  n_alive is zeroed and afterwards holds the episodes still alive after last_step.
 *   Both forms run the same action norm and the same bookkeeping on the same env step, so EVERY kp1_eval_buffers array -- the action-norm
 * columns included -- is bit-equal to the one the same steps made by kp1_eval_step leave, for any split of [1, limit] into consecutive calls
 * (tests/test_eval_episodes_gpu.py).
 *   One deliberate difference in the env handle: an episode that has ended (or was never active) is NOT stepped again, whereas kp1_eval_step
 * steps every row for as long as the host keeps calling it.  After the call env i has been stepped counters[0][i] - (its count at entry)
 * times; its handle fields, observation row, reward[i] and done[i] are those of its last step, whatever its neighbours did; a row that was
 * never alive is untouched, and so is everything of a tile without a live episode. */
#define KP1_EVAL_EPISODES_MAX_STEPS 256
int kp1_eval_episodes(kp1_mlp* m, kp1_env* env, float* obs, float* reward, uint8_t* done, const kp1_eval_buffers* buffers,
                      int32_t first_step, int32_t last_step, const double* ready_thresholds /* [4] or NULL */, int32_t confirm_steps, void* stream);

/* one PPO minibatch: forward + loss + full backward.  Rows are gathered through idx (int64 [n] into the [total] axis, or
 * NULL = rows 0..n).  grad_out f32 [num_params] receives d loss / d params in SB3 order (overwritten), with
 *   loss = sum_i[-min(r_i A_i, clip(r_i, 1-c, 1+c) A_i)] * inv_count + vf_coef * sum_i (R_i - V_i)^2 * inv_count - ent_coef * H,
 * r = exp(logp - old_logp), H = entropy of the diagonal Gaussian (state independent).
 * stats_out f32[4] += (policy_loss, value_loss, entropy, approx_kl) of this minibatch.
 * Every producer kernel writes per-workgroup partials with plain stores and one finalize kernel sums them in a fixed order:
 * no float atomics touch a gradient, results are bitwise reproducible.  grad_is_zero is accepted for ABI stability and ignored. */
int kp1_mlp_loss_grad(kp1_mlp* m, const float* obs, int32_t obs_stride, const int64_t* idx, int32_t n, const float* actions,
                      const float* old_log_prob, const float* advantages, const float* returns, float adv_mean, float adv_inv_std,
                      const float* adv_stats_dev, float clip_range, float ent_coef, float vf_coef, float inv_count, float* grad_out,
                      float* stats_out, int32_t grad_is_zero, void* stream);

/* Options.  KP1_MLP_OPT_FUSED (default 1): for hidden = 256, kp1_mlp_loss_grad runs layer 1, layer 2, the heads, the PPO loss
 * and the activation backward of a 32-row minibatch tile in one workgroup (mlp_tile_kernel<true>) instead of four
 * chip-synchronous launches, and kp1_mlp_forward runs layer 1, layer 2, the heads and the Gaussian sampling in one launch
 * (mlp_tile_kernel<false>) instead of three; 0 selects the layer-wise kernels.  Hidden 64 / 128 handles do not read this option: they run
 * the layer-wise kernels, or train_tile128_kernel under KP1_MLP_OPT_TRAIN_TILE.  Same results up to fp32 summation order of the per-tile
 * partials. */
#define KP1_MLP_OPT_FUSED 1
/* KP1_MLP_OPT_ACTOR_EXTRA_STEPS (default 0): optimiser steps the actor tensors (mlp_extractor.policy_net.*, action_net.*) have taken
 * on top of the common count -- torch.optim.Adam counts per tensor, and the route trainer's teacher-anchor callback
 * (route/teacher_anchor.py:68-87) steps only the tensors its imitation loss reaches.  kp1_mlp_adam_step uses common + extra in
 * the bias corrections of those tensors. */
#define KP1_MLP_OPT_ACTOR_EXTRA_STEPS 2
/* KP1_MLP_OPT_STEP_COUNT: set the device-resident optimiser step count (PPO.load restores torch.optim.Adam's state, whose per-tensor
 * `step` feeds the bias corrections); kp1_mlp_loss_grad increments it, kp1_mlp_adam_step(step = 0) reads it. */
#define KP1_MLP_OPT_STEP_COUNT 3
/* KP1_MLP_OPT_PROFILE (default 0): attach a HIP-event pair to every kernel launch of the optimiser step (the dispatch's own begin and end),
 * on the launch stream and in the real launch sequence, so that a kernel's average duration is measured in situ (caches in the state the previous kernel of the
 * step left them) rather than in a back-to-back micro loop.  kp1_mlp_profile_read waits for the recorded launches and returns, per
 * slot, the average duration in microseconds and the launch count since the last read.  Not usable while a hipGraph is being captured. */
#define KP1_MLP_OPT_PROFILE 4
/* KP1_MLP_OPT_BF16X3_WGRAD (default 0) -- EXPERIMENT, not the measured product path: the weight-gradient GEMMs dW2 = dZ2^T h1, dW1 = dZ1^T X on
 * operands the tile kernel pre-splits into three bf16 pieces (x = hi + mid + lo, 24 bits) and six bf16 MFMAs per product block, fp32 accumulation
 * (gemm_tn_bf16x3_kernel) instead of the exact fp32 MFMA kernel.  Not bit-identical to the exact path: error table in DESIGN.md / bench.py's
 * `experiment_bf16x3_wgrad` block.  bench.py's `value` and `dtype` never use it. */
#define KP1_MLP_OPT_BF16X3_WGRAD 5
/* KP1_MLP_OPT_TRAIN_TILE (default 0): hidden 64 / 128 handles (K = 1 or a population, obs_dim 56 or 80).  While it is on, kp1_mlp_loss_grad of
 * a minibatch of n <= 2048 rows per replica launches [adv_partials ->] train_tile128_kernel -> grad_finalize where it launched the five
 * layer-wise kernels (two forward GEMMs, the head kernel, the backward GEMM, two weight-gradient GEMMs): a workgroup carries one 32-row tile
 * of one net through forward, loss and backward and leaves one partial of every gradient.  A larger n takes the layer-wise launches.  Every
 * argument of kp1_mlp_loss_grad behaves as documented; stats_out and the gradients of log_std, action_net, value_net and the layer-2 biases
 * are bit-equal to the layer-wise result, the weight and layer-1 bias gradients are other fp32 sums of the same terms.  A hidden 256 handle
 * returns KP1_ERR_UNSUPPORTED (its tile path is KP1_MLP_OPT_FUSED).  KP1_MLP_PROFILE_TILE times the launch. */
#define KP1_MLP_OPT_TRAIN_TILE 6
#define KP1_MLP_PROFILE_SLOTS 4
#define KP1_MLP_PROFILE_TILE 0      /* mlp_tile_kernel<true, .>: forward + loss + activation backward of both nets; train_tile128_kernel */
#define KP1_MLP_PROFILE_WGRAD 1     /* gemm_tn_frag_kernel: dW2 + dW1 of both nets */
#define KP1_MLP_PROFILE_FINALIZE 2  /* grad_finalize_kernel */
#define KP1_MLP_PROFILE_ADAM 3      /* (sum of squares +) adam_kernel */
int kp1_mlp_set_option(kp1_mlp* m, int32_t option, int32_t value);
int kp1_mlp_profile_read(kp1_mlp* m, float* out_us /* [KP1_MLP_PROFILE_SLOTS] */, int32_t* out_launches /* [KP1_MLP_PROFILE_SLOTS] */);

/* clip_grad_norm_(max_norm) + Adam(beta 0.9/0.999, eps) step on the flat vectors; the same pass repacks the kernel-format
 * weights.  step = 1-based Adam step count, or <= 0 to use the device-resident counter that every kp1_mlp_loss_grad call
 * increments (needed when the call sequence is replayed from a hipGraph).  flags bit 1 (value 2): grad is untouched since the kp1_mlp_loss_grad call that
 * produced it (no all-reduce in between), so the norm partials that call left are reused instead of a reduction launch. */
int kp1_mlp_adam_step(kp1_mlp* m, float* params, float* grad, float* exp_avg, float* exp_avg_sq, float lr, float eps,
                      float max_grad_norm, int32_t step, int32_t flags, void* stream);

/* ---- KL early stop (SB3 PPO's target_kl) as a device decision, per replica ---------------
 * SB3's train() leaves its epochs once a minibatch's approx_kl exceeds 1.5 * target_kl: that minibatch's loss terms are logged, its
 * optimiser step and everything after it are not taken.  An update replayed from a hipGraph cannot ask the host, so the handle keeps one
 * record per replica and, while a gate is set, kp1_mlp_loss_grad and kp1_mlp_adam_step launch the gated forms of their last kernels:
 *   finalize  the gradient and the norm partials as always.  A replica that has not stopped adds the minibatch to stats_out and counts it;
 *             then, if (double)kl > threshold with kl = (KL sum) * inv_count as a float -- exactly what a zeroed stats_out[3] would receive --
 *             it stops (stop_index = n_seen, stop_kl = kl), otherwise it advances ITS Adam step count.  A stopped replica adds nothing to
 *             stats_out.  n_seen advances in every launch.
 *   Adam      a stopped replica's launch returns before any store; the others step on their own count.
 * The tile, GEMM and head kernels in front of them run as before (after a stop they compute a gradient nobody uses).  The step count is
 * kept per replica from the moment a gate is set: KP1_MLP_OPT_STEP_COUNT then sets every replica's, kp1_mlp_kl_gate_read returns them. */
typedef struct kp1_kl_gate {
  double threshold;    /* 1.5 * target_kl, formed on the host; +inf = this replica never stops */
  int32_t stopped;     /* 1 from the stopping minibatch on */
  int32_t n_counted;   /* minibatches whose statistics entered stats_out since the gate was armed (the stopping one included) */
  int32_t n_seen;      /* kp1_mlp_loss_grad calls since the gate was armed */
  int32_t stop_index;  /* n_seen at the stopping minibatch, 0-based */
  float stop_kl;       /* its approx_kl */
  int32_t reserved0;
} kp1_kl_gate;
/* Set (n = K: one target per replica, host memory; NaN or <= 0 = no target for that replica) or clear (n = 0; target_kl_host may be NULL)
 * the gate of a handle.  Setting it arms every record and, if no gate was set, gives every replica the handle's step count.  Refused
 * before anything is written: NULL arguments, n other than 0 or K, a handle whose KP1_MLP_OPT_ACTOR_EXTRA_STEPS is non-zero, a `stream`
 * that is being captured, and clearing while the replicas' step counts differ (KP1_ERR_INVALID: one shared count cannot hold them).
 * While a gate is set kp1_mlp_anchor_loss_grad / kp1_mlp_anchor_adam_step return KP1_ERR_UNSUPPORTED (they read the shared count) and
 * KP1_MLP_OPT_ACTOR_EXTRA_STEPS refuses a non-zero value.  Waits for `stream`. */
int kp1_mlp_set_kl_gate(kp1_mlp* m, const double* target_kl_host, int32_t n, void* stream);
/* a new train() call: clears stopped, n_counted, n_seen, stop_index and stop_kl of every replica in one launch (capturable) */
int kp1_mlp_kl_gate_arm(kp1_mlp* m, void* stream);
/* copy the K records and the K step counts to the host (either may be NULL); waits for `stream` */
int kp1_mlp_kl_gate_read(kp1_mlp* m, kp1_kl_gate* out_host, int32_t* out_steps, void* stream);

/* The route trainer's teacher-anchor side loss as a device step (handles on the layer-wise path: hidden 64 or 128, K = 1 or a population;
 * hidden 256 returns KP1_ERR_UNSUPPORTED).  For replica k
 *   loss_k = loss_weight * mean_{i < n, d < 7} (mean_k(obs[idx[k][i]])_d - teacher_actions[idx[k][i]][d])^2
 * on the unclipped deterministic policy mean.  obs [M][obs_stride] and teacher_actions [M][7] are the shared dataset; idx is int64 [K][n]
 * for a population (required) and [n] or NULL (rows 0..n) for K = 1.  grad_out f32 [K][num_params] is overwritten: the gradient of the six
 * actor tensors (mlp_extractor.policy_net.{0,2}.{weight,bias}, action_net.{weight,bias}), 0 everywhere else.  loss_out f32 [K] is
 * overwritten.  Partials are summed in a fixed order (no float atomics): bitwise reproducible.  Unlike kp1_mlp_loss_grad it does NOT advance
 * the device-resident step count. */
int kp1_mlp_anchor_loss_grad(kp1_mlp* m, const float* obs, int32_t obs_stride, const int64_t* idx, int32_t n, const float* teacher_actions,
                             float loss_weight, float* grad_out, float* loss_out, void* stream);

/* clip_grad_norm_(max_grad_norm) over the six actor tensors + Adam(beta 0.9/0.999) on those tensors only, for the gradient the preceding
 * kp1_mlp_anchor_loss_grad call on this handle wrote (its norm partials are reused).  The bias corrections use the step count
 * common + actor_extra + 1: common = step if step > 0, else the device-resident counter; actor_extra = the KP1_MLP_OPT_ACTOR_EXTRA_STEPS value.
 * No other element of params / exp_avg / exp_avg_sq is written; the kernel-format weights of the changed elements are repacked.  With a
 * replica hyper-parameter table set, replica k uses its learning_rate and adam_eps; the norm bound is always the argument.  Afterwards
 * actor_extra is one larger (stream ordered, so a kp1_mlp_adam_step replayed from an already captured graph sees it). */
int kp1_mlp_anchor_adam_step(kp1_mlp* m, float* params, float* grad, float* exp_avg, float* exp_avg_sq, float lr, float eps,
                             float max_grad_norm, int32_t step, void* stream);

/* HIP-event timing of the MFMA kernels at minibatch size n (for bench.py's roofline block): runs each kernel `iters` times back
 * to back on `stream` between hipEventRecord pairs and returns the mean duration in milliseconds (out_ms / out_flops hold 6):
 *   out_ms[0] gemm_nt fwd layer 2 (H x H, bias+tanh)    out_ms[1] gemm_nt bwd dZ1 (H x H, dtanh)
 *   out_ms[2] gemm_tn dW2 (H x H, split over the batch)  out_ms[3] gemm_nt fwd layer 1 (64 -> H)
 *   out_ms[4] mlp_tile_kernel<true> (hidden 256: layer 1 + layer 2 + heads + loss + activation backward of both nets)
 *   out_ms[5] gemm_tn_frag_kernel (hidden 256: dW2 + dW1 of both nets)          [4], [5] = 0 for other widths
 * out_flops[k] = algorithmic FLOPs of one launch of kernel k (2*M*N*K summed over its GEMMs and both nets). */
/* Placement self-check of the two SPEED assumptions of the update kernels (never correctness): launches a probe with the training tile's launch
 * shape for an n_rows minibatch and reports where the hardware put the workgroups.  out[8] (host): [0] workgroups, [1] pairs (k, k + #CUs) probed,
 * [2] of them on the same CU (what the tile kernel's 12 us stagger assumes), [3] workgroups that run on the XCD of workgroup (linear index % 8)
 * and [7] distinct XCDs among workgroups 0..7 (what the weight-gradient kernel's chunk-major block order assumes: [3] = all, [7] = 8),
 * [4] #CUs, [5] distinct CUs used, [6] workgroups that arrived while the probe waited. */
int kp1_mlp_placement_check(int32_t device, int32_t n_rows, int32_t* out, void* stream);
int kp1_mlp_time_kernels(kp1_mlp* m, const float* obs, int32_t obs_stride, int32_t n, int32_t iters, float* out_ms, double* out_flops,
                         void* stream);

/* make kp1_step / kp1_reset write observation rows with this stride (56 default, 64 = MFMA-friendly, zero padded) */
int kp1_set_obs_stride(kp1_env* env, int32_t stride);

/* ---- device-resident training monitor: SB3's episode statistics (common/monitor.py Monitor.step +
 * OnPolicyAlgorithm._update_info_buffer) and explained variance, fed from the rollout buffers --------------------
 * make_vec_env wraps every env in a Monitor, which sums an episode's rewards and counts its steps; when the episode ends
 * the (return, length) pair enters ep_info_buffer, a deque(maxlen = stats_window_size), whose mean SB3 logs as
 * rollout/ep_rew_mean and rollout/ep_len_mean.  Here K replicas x N envs keep that state on the device: per env a carry (running return
 * as double, running length as int32), per replica one kp1_monitor_state -- the ring of the newest `window` episodes and two totals. */
#define KP1_MONITOR_MAX_WINDOW 1024
#define KP1_MONITOR_MAX_STEPS 4096   /* largest max_steps of a handle (twice the longest n_steps of a committed config) */
typedef struct kp1_monitor_state {
  int32_t window, ring_len, ring_head, reserved0;   /* live entries: the ring_len slots from ring_head on (ring_head is 0 while the ring fills) */
  int64_t total_episodes, total_successes;
  double  ring_return[KP1_MONITOR_MAX_WINDOW];
  int32_t ring_length[KP1_MONITOR_MAX_WINDOW];
  uint8_t ring_success[KP1_MONITOR_MAX_WINDOW];
} kp1_monitor_state;
typedef struct kp1_monitor kp1_monitor;

/* window in [1, KP1_MONITOR_MAX_WINDOW] (SB3's stats_window_size, default 100), n_replicas in [1, KP1_CURRICULUM_MAX_REPLICAS],
 * n_per_replica >= 1, max_steps in [1, KP1_MONITOR_MAX_STEPS] = the largest T of an observe call (sizes the scratch). */
int kp1_monitor_create(int32_t device, int32_t n_replicas, int32_t n_per_replica, int32_t window, int32_t max_steps, kp1_monitor** out);
int kp1_monitor_destroy(kp1_monitor* mon);
/* Feed T env steps: rewards f32 and dones u8 (KP1_DONE_* bits), both [T][K N], time-major with replica-major columns (the rollout buffers),
 * 1 <= T <= max_steps.  Env i's episode ends at step t when dones[t][i] & (TERMINATED | TRUNCATED) (kp1_gae_scan's test); its return is the
 * carry plus the rewards of its steps, each widened to double and added in step order, its length the number of those steps, its success
 * KP1_DONE_SUCCESS of that byte; then the carry is zero again.  Replica k's episodes of the call enter its ring in (t, then env index)
 * order -- the order the reference's callbacks and SB3's deque see -- and the ring keeps the newest `window`.  Two calls over [0, a) and
 * [a, T) leave the states and carries exactly as one call over [0, T).  Two launches, no float atomics, one writer per element. */
int kp1_monitor_observe(kp1_monitor* mon, const float* rewards, const uint8_t* dones, int32_t T, void* stream);
/* clear the carries (after an explicit env reset: the running episodes were abandoned); rings and totals stay */
int kp1_monitor_reset_carry(kp1_monitor* mon, void* stream);
/* copy replica `replica`'s state to the host (waits for the stream) */
int kp1_monitor_read(kp1_monitor* mon, int32_t replica, kp1_monitor_state* out_host, void* stream);

/* stable_baselines3.common.utils.explained_variance's two variances per replica, in ONE launch: values / returns f32 [T][n_total] (the same
 * layout; n_total = K n_per_replica), out f64 [K][2] (device) = (var(returns), var(returns - values)), population variances (np.var) of
 * the inputs widened to double, accumulated in double as (sum, sum of squares) of the data shifted by the replica's first element, in a
 * fixed order.  The host forms 1 - var_diff / var_y, nan when var_y == 0.  T * n_total < 2^31. */
int kp1_explained_variance(int32_t device, const float* values, const float* returns, int32_t T, int32_t n_total, int32_t n_per_replica,
                           double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KP1_PPO_H */
