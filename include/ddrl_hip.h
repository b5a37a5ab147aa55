/* ddrl_hip.h -- C-ABI of libddrl_hip.so, the MI355X (gfx950) hot path of DDRL.
 *
 * This boundary replaces the numeric work that the reference delegates to RLlib 1.0.x and
 * TensorFlow 2.3, which run behind two plugin interfaces:
 *   (1) MultiAgentEnv: simulation_envs/quantruped_adaptor_multi_environment.py:8-272
 *       (distribute_observations :124-136, distribute_reward :173-203,
 *        concatenate_actions :205-212, step :220-250)
 *   (2) ModelV2: models/fcnet_glorot_uniform_init.py:10-125 ("ffn"),
 *       models/shared_graphnet_glorot_uniform_init.py:14-58 + graph_net.py + gcn.py ("gnn"),
 *       registered in models/__init__.py:7-13.
 * The RLlib side they plug into (sampling, GAE, PPOLoss, clip_gradients, Adam, minibatch
 * SGD, KL update) is rebuilt here as HIP kernels.  Host code -- Python through ctypes, or a
 * maintainer's own FFI binding -- drives these entry points.
 *
 * Conventions
 *   - Every function returns int status: 0 = OK, < 0 = error; ddrl_last_error() returns a
 *     thread-local message.  No exceptions cross the boundary.
 *   - Pointers named *_dev are device (HBM) pointers.  Pointers named *_host are host
 *     memory (pageable or pinned).  Work is enqueued on the context's stream
 *     (ddrl_set_stream) and is asynchronous unless stated otherwise.
 *   - One context = one device + one stream; calls on a context are serialized by the caller.
 */
#ifndef DDRL_HIP_H
#define DDRL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDRL_ABI_VERSION 4
#define DDRL_MAX_POLICIES 4
#define DDRL_MAX_AGENTS 4
#define DDRL_MAX_OBS 48

enum { DDRL_MODEL_FFN = 0, DDRL_MODEL_GNN = 1 };
enum { DDRL_REWARD_PER_LEG = 0, DDRL_REWARD_GLOBAL = 1, DDRL_REWARD_NORM = 2 };
enum { DDRL_VF_CLIP_RAY10 = 0, DDRL_VF_CLIP_SQUARED = 1 };
/* message-passing layer of the "gnn" model (models/graph_net.py:20 selects one of
 * models/gcn.py's layers: MPNN :39-94 (the reference's default), GCN :7-37, MPNN2 :96-150,
 * GAT1 :153-206) */
enum { DDRL_GNN_MPNN = 0, DDRL_GNN_GCN = 1, DDRL_GNN_MPNN2 = 2, DDRL_GNN_GAT1 = 3 };

/* Static configuration of one context (one env shard of one trainer). */
typedef struct ddrl_cfg {
  int32_t n_envs;        /* N: parallel environments on this device                      */
  int32_t frag_len;      /* T: rollout_fragment_length                                     */
  int32_t obs_full_dim;  /* 43 (44 with target velocity)                                   */
  int32_t n_agents;      /* agents per env: 4 (legs), 2 (sides/diagonals), 1 (centralized) */
  int32_t n_policies;    /* P                                                              */
  int32_t model_kind;    /* DDRL_MODEL_FFN | DDRL_MODEL_GNN                               */
  int32_t act_dim;       /* A: actions per agent (2, 4 or 8)                               */
  int32_t agent_policy[DDRL_MAX_AGENTS];           /* policy id of every agent            */
  int32_t obs_dim[DDRL_MAX_POLICIES];              /* d per policy (GNN: 19 per node)      */
  int32_t obs_index[DDRL_MAX_AGENTS][DDRL_MAX_OBS];/* gather table per agent (a1); entries
                                                      -1 / -2 are the constants 0 / 1 (the
                                                      one-hot leg id of the LegID env)      */
  int32_t act_index[DDRL_MAX_AGENTS][8];           /* scatter table per agent (a7)         */
  int32_t n_contact[DDRL_MAX_AGENTS];              /* contact-cost bodies per agent (a8)   */
  int32_t contact_index[DDRL_MAX_AGENTS][14];
  float contact_weight[DDRL_MAX_AGENTS][14];
  float leg_angle_deg[DDRL_MAX_AGENTS];            /* GNN ego encoding (FL,HL,HR,FR)       */
  int32_t filter_enabled;   /* env-side MeanStdFilter on the full observation (a2)         */
  int32_t filter_update;    /* push batches into the running statistics                   */
  float filter_clip;        /* 10 in the reference; 0 = no clip                            */
  int32_t reward_mode;      /* DDRL_REWARD_*                                                */
  float ctrl_cost_weight;
  float contact_cost_weight;
  float gamma, lambda_;
  float clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff;
  float lr, grad_clip;
  float adam_beta1, adam_beta2, adam_eps;
  int32_t vf_clip_mode;     /* DDRL_VF_CLIP_*                                               */
  int32_t sgd_minibatch_size;  /* 128, or 256 for the fcnet models (the sizes the fused    */
                               /* update kernels are built for); anything else is refused  */
  int32_t num_sgd_iter;        /* 10                                                       */
  int32_t act_negate[DDRL_MAX_AGENTS][8];  /* 1: negate action j of the agent in the env action
                                              vector (LegTransforms: fr / hr knee)          */
  int32_t policy_filter;    /* RLlib observation_filter "MeanStdFilter" on every policy's
                               input (after the env-side filter; unclipped, fp64 stats)     */
  int32_t leg_coupling;     /* "cup" model (models/coupling_net_glorot_uniform_init.py:11-30,
                               registered models/__init__.py:10): the action means of the
                               shared leg policy are scaled by a trainable table [4][A],
                               row = the agent's leg index (SharedDecentralLegID env, :66-114);
                               the table follows the fcnet variables in the parameter vector */
  int32_t gnn_layer;        /* DDRL_GNN_* (model_kind GNN): the layer's kernels sit between the
                               state encoder and linear_out of each net, in Keras order */
} ddrl_cfg;

typedef struct ddrl_ctx ddrl_ctx;

int ddrl_abi_version(void);
const char* ddrl_last_error(void);

/* Context lifetime.  Allocates every device buffer for T x N rollouts. */
int ddrl_ctx_create(const ddrl_cfg* cfg, int device, ddrl_ctx** out);
int ddrl_ctx_destroy(ddrl_ctx* ctx);
int ddrl_set_stream(ddrl_ctx* ctx, void* hip_stream);
int ddrl_synchronize(ddrl_ctx* ctx);

/* Shapes.  layout_out[11] = {row_stride, off_obs, off_act, off_logits, off_logp, off_vf,
 * off_adv, off_vt, off_rew, rows_per_step (C = N*k), off_leg (leg index of the row, "cup"
 * model; -1 otherwise)}, all in floats. */
int ddrl_param_count(ddrl_ctx* ctx, int pid, int64_t* n_out);
int ddrl_record_layout(ddrl_ctx* ctx, int pid, int32_t* layout_out);

/* Parameter / optimizer / filter state, in the reference's Keras checkpoint order
 * (pid/fc_1/kernel [d,64], fc_1/bias, fc_value_1/..., fc_2/..., fc_value_2/...,
 *  fc_out/..., value_out/...), replacing Policy.get_weights/set_weights. */
int ddrl_params_set(ddrl_ctx* ctx, int pid, const float* host, size_t n);
int ddrl_params_get(ddrl_ctx* ctx, int pid, float* host, size_t n);
int ddrl_adam_set(ddrl_ctx* ctx, int pid, const float* m_host, const float* v_host, size_t n,
                  float beta1_power, float beta2_power);
int ddrl_adam_get(ddrl_ctx* ctx, int pid, float* m_host, float* v_host, size_t n,
                  float* beta1_power, float* beta2_power);
int ddrl_filter_set(ddrl_ctx* ctx, double n, const double* mean_host, const double* sq_host);
int ddrl_filter_get(ddrl_ctx* ctx, double* n, double* mean_host, double* sq_host);
/* Pushes since the last ddrl_filter_delta_reset, as their own running stat (RLlib's filter
 * "buffer"); a data-parallel trainer merges every rank's delta into the synced filter
 * (RunningStat.update in rank order) and resets (synchronize_filters, P_Local:160). */
int ddrl_filter_delta_get(ddrl_ctx* ctx, double* n, double* mean_host, double* sq_host);
int ddrl_filter_delta_reset(ddrl_ctx* ctx);
/* The per-policy RLlib MeanStdFilter (cfg.policy_filter): RunningStat of policy pid over its
 * obs_dim input columns, and its pushes since the last delta reset (same sync protocol). */
int ddrl_policy_filter_set(ddrl_ctx* ctx, int pid, double n, const double* mean_host, const double* sq_host);
int ddrl_policy_filter_get(ddrl_ctx* ctx, int pid, double* n, double* mean_host, double* sq_host);
int ddrl_policy_filter_delta_get(ddrl_ctx* ctx, int pid, double* n, double* mean_host, double* sq_host);
int ddrl_policy_filter_delta_reset(ddrl_ctx* ctx);

/* Rollout (per env step).
 * observe: env-side MeanStdFilter push + normalize + per-agent routing of the raw
 *          observations obs_dev[N][obs_full_dim] (a1/a2/a3).
 * act:     fused forward of every policy on the routed observations, DiagGaussian sample
 *          with explicit noise eps_dev[N][n_agents][A], logp, value; writes training row
 *          t and the clipped env actions actions_dev[N][8] (a4/a6/a7).
 * reward:  per-agent rewards for row t from forward reward fw_dev[N], contact forces
 *          cfrc_dev[N][14][6], the env actions and done flags done_dev[N] (a8).
 * bootstrap: V(s_T) of the routed observations -> last values for GAE. */
int ddrl_observe(ddrl_ctx* ctx, const float* obs_dev);
int ddrl_act(ddrl_ctx* ctx, int t, const float* eps_dev, float* actions_dev);
int ddrl_reward(ddrl_ctx* ctx, int t, const float* fw_dev, const float* cfrc_dev,
                const float* actions_dev, const uint8_t* done_dev);
int ddrl_bootstrap(ddrl_ctx* ctx);
/* The same over the envs [e0, e1) only, on full-size buffers (obs_dev[N][D], eps_dev, actions_dev,
 * fw_dev, cfrc_dev, done_dev): a pipelined host env plane (ddrl_rollout_hostenv) runs its env
 * groups through these so that one group's host step overlaps another group's device work.
 * The env-side filter pushes the range's rows as one batch (groups in call order). */
int ddrl_observe_range(ddrl_ctx* ctx, const float* obs_dev, int e0, int e1);
int ddrl_act_range(ddrl_ctx* ctx, int t, int e0, int e1, const float* eps_dev, float* actions_dev);
int ddrl_reward_range(ddrl_ctx* ctx, int t, int e0, int e1, const float* fw_dev, const float* cfrc_dev,
                      const float* actions_dev, const uint8_t* done_dev);
/* A whole fragment over device-resident env data (a device env, replayed transitions, the
 * synthetic benchmark): for t in [0, T): act(t), reward(t), observe(obs_dev[t + 1]); then
 * bootstrap.  Expects observe(obs_dev[0]) to have been called.  Layouts: obs_dev[T+1][N][D],
 * eps_dev[T][N][n_agents][A], fw_dev[T][N], cfrc_dev[T][N][14][6], done_dev[T][N] (may be
 * NULL), actions_dev[N][8] (scratch: the env actions of the last step).  One call instead of
 * 3 T host calls: the per-step launches stay in C++, captured once into a HIP graph that is
 * re-launched while the six buffer pointers are unchanged (contents may change between calls;
 * DDRL_ROLLOUT_GRAPH=0 at context creation issues the launches directly). */
int ddrl_rollout_fragment(ddrl_ctx* ctx, const float* obs_dev, const float* eps_dev, const float* fw_dev,
                          const float* cfrc_dev, const uint8_t* done_dev, float* actions_dev);
/* Host-buffer variants for a host-side env (MultiAgentEnv.step on host cores): pinned
 * buffers, hipMemcpyAsync on the context's stream, asynchronous like the device calls.
 *   step_host:     obs_host[N][D] in -> observe; eps_host in -> act(t); actions_host[N][8] out
 *                  (the reset observation and the first action of a fragment);
 *   act_host:      eps_host in -> act(t) on the staged observation -> actions_host out;
 *   env_step_host: the env's answer to the actions of step t: fw_host[N], cfrc_host[N][14][6],
 *                  done_host[N] (may be NULL) -> reward(t); obs_next_host[N][D] -> observe.
 * A loop over t: act_host(t) (step_host for t = 0), synchronize, step the envs on the host,
 * env_step_host(t). */
int ddrl_step_host(ddrl_ctx* ctx, int t, const float* obs_host, const float* eps_host,
                   float* actions_host);
int ddrl_act_host(ddrl_ctx* ctx, int t, const float* eps_host, float* actions_host);
int ddrl_env_step_host(ddrl_ctx* ctx, int t, const float* fw_host, const float* cfrc_host,
                       const uint8_t* done_host, const float* obs_next_host);

/* f1 host env plane (hostenv.cpp): a vectorized QuAntruped stand-in (clean-room kinematics in
 * the reference env's layout -- MuJoCo is absent; see hostenv.h) stepped by a pool of
 * n_threads host threads into pinned buffers obs[N][obs_dim], act[N][8], fw[N],
 * cfrc[N][14][6], done[N] (ddrl_hostenv_buffers).  Replaces the reference's per-worker
 * MuJoCo stepping (simulation_envs/quantruped_v3.py:166-267) and the adaptor's
 * step(action_dict) (quantruped_adaptor_multi_environment.py:220-250).
 *   step: the envs [e0, e1) with act[e][8] (clipped to [-1, 1]); a done env is reset at once.
 * ddrl_rollout_hostenv runs a whole fragment over it, pipelined over `groups` env groups (one
 * group's host step overlaps the other groups' device work and transfers), then bootstraps. */
typedef struct ddrl_hostenv ddrl_hostenv;
const char* ddrl_hostenv_last_error(void);
int ddrl_hostenv_create(int n_envs, int obs_dim, int n_threads, uint64_t seed, float target_velocity,
                        ddrl_hostenv** out);
int ddrl_hostenv_destroy(ddrl_hostenv* env);
int ddrl_hostenv_buffers(ddrl_hostenv* env, float** obs, float** act, float** fw, float** cfrc, uint8_t** done);
int ddrl_hostenv_reset(ddrl_hostenv* env);
int ddrl_hostenv_step(ddrl_hostenv* env, int e0, int e1);
int ddrl_hostenv_threads(ddrl_hostenv* env);
/* Target velocities of the TVel envs (obs_dim 44): every env draws its episode's velocity
 * uniformly from list[0..n) on every reset, the adaptor's random.choice(target_velocity_list)
 * at construction and in reset() (quantruped_adaptor_multi_environment.py:47-50, 214-216); the
 * draw takes effect at the next reset (ddrl_hostenv_reset, or an episode end).  create's
 * target_velocity is the list of one.  target_velocities: each env's current velocity. */
int ddrl_hostenv_set_target_velocities(ddrl_hostenv* env, const float* list, int n);
int ddrl_hostenv_target_velocities(ddrl_hostenv* env, float* out, int n_envs);
/* update_environment_after_epoch (quantruped_adaptor_multi_environment.py:97-122, after every
 * training iteration through on_train_result, train_experiment_1_architecture_on_flat.py:171-178):
 * every env's state and TimeLimit count restart (gym env.reset()), the target velocity is kept,
 * no done flag is raised and obs is not rewritten (the adaptor discards that observation).
 * The terrain regeneration of the same hook is ddrl_hostenv_new_terrain (below). */
int ddrl_hostenv_reset_state(ddrl_hostenv* env);
/* Uneven ground (the reference's hf_smoothness and create_new_hfield, quantruped_v3.py:25-54): a
 * procedural height field, a pure function of (seed, env index, generation, the env's episode
 * number, smoothness, x, y) with no stored map -- a lattice of uniform values every bump_scale
 * metres, smoothstep-interpolated, cleared to exactly 0.0 on the start patch max(|x|, |y|) <= 0.8
 * and rising to full height at 2.4 (csrc/envdyn.h states the operation order; both planes compute
 * it bit for bit alike).  Each foot's contact height is lowered by the field under that foot.
 *   set_terrain: every env draws its smoothness from [lo, hi] per generation (lo == hi: fixed);
 *     1 is flat, 0 the roughest (heights in [0, 1 - smoothness]).  Refuses anything outside
 *     0 <= lo <= hi <= 1 and bump_scale > 0.  Defaults: 1, 1, 2.0 (the reference's hf_bump_scale),
 *     generation 0.  With lo == hi == 1 the step is the flat one, unchanged.
 *   new_terrain: create_new_random_hfield -- generation += 1, new ground for every env.  Within a
 *     generation every episode of an env has its own ground as well (the field is keyed by the
 *     episode number; the reference makes a new field before every evaluation episode).
 *   terrain_height: the probe -- out[i] = the height of env env_index[i]'s current ground at
 *     (xy[2i], xy[2i + 1]). */
int ddrl_hostenv_set_terrain(ddrl_hostenv* env, double lo, double hi, double bump_scale, uint32_t generation);
int ddrl_hostenv_terrain(ddrl_hostenv* env, double* lo, double* hi, double* bump_scale, uint32_t* generation);
int ddrl_hostenv_new_terrain(ddrl_hostenv* env);
int ddrl_hostenv_terrain_height(ddrl_hostenv* env, const int32_t* env_index, const double* xy, int n, double* out);
int ddrl_rollout_hostenv(ddrl_ctx* ctx, ddrl_hostenv* env, int groups, const float* eps_dev, int reset);
/* What evaluation needs of the env plane.
 *   kin: the pinned buffer kin[N][9] = {torso dx of the step, joint velocities qd[0..7]}, written
 *     by step before a done env is reset (the observation of a done step is the reset one);
 *   set_time_limit: the TimeLimit of every env (default 1000), the reference's
 *     `while not done and steps < num_steps` (evaluation/rollout_episodes.py:83);
 *   reset_episodes: every env starts a fresh episode at step 0 -- target velocity drawn,
 *     observation written, done cleared (ddrl_hostenv_reset staggers the episode phases). */
int ddrl_hostenv_kin(ddrl_hostenv* env, float** kin);
int ddrl_hostenv_set_time_limit(ddrl_hostenv* env, int steps);
int ddrl_hostenv_reset_episodes(ddrl_hostenv* env);
/* The packed fp64 state of every env, DDRL_ENV_STATE_DOUBLES doubles per env, env-major:
 *   [0..9]   torso {x, y, z, vx, vy, vz, roll, pitch, wroll, wpitch}
 *   [10..17] joint angles q, [18..25] joint velocities qd, [26..33] last joint forces qfrc
 *            (joints: FL hip, FL knee, HL hip, HL knee, HR hip, HR knee, FR hip, FR knee)
 *   [34..37] last contact force per foot, [38] steps of the episode, [39] episode number,
 *   [40]     target velocity of the episode.
 * n == n_envs * DDRL_ENV_STATE_DOUBLES.  state_set replaces the state only: the output buffers
 * (obs, fw, cfrc, kin, done) keep their contents until the next step.  The device env plane
 * (below) exchanges the same layout, so a running env can be handed from one plane to the other. */
#define DDRL_ENV_STATE_DOUBLES 41
int ddrl_hostenv_state_get(ddrl_hostenv* env, double* host, size_t n);
int ddrl_hostenv_state_set(ddrl_hostenv* env, const double* host, size_t n);

/* Device env plane (devenv.hip): the same stand-in dynamics (one source, csrc/envdyn.h) stepped by a
 * HIP kernel on the context's stream, four lanes per env (one per leg), the state in device
 * memory.  Bound to a context: device, stream, n_envs and obs_full_dim (43 or 44) are the
 * context's.  It emits the host plane's buffers in device memory (ddrl_devenv_buffers):
 * obs[N][D], fw[N], cfrc[N][14][6], kin[N][9] (written before a done env is reset), done[N].
 * Every call below is asynchronous on the context's stream unless it says otherwise, and
 * reports through ddrl_last_error().  Integer arithmetic, the hash, + - * / and the conversions
 * match the host plane bit for bit (the kernels are built without fp contraction); sin / cos are
 * the device library's and may differ from the host's in the last places, which reaches the torso
 * state and the foot forces but not the joints ("Device env plane").
 *   create: seed and target_velocity as ddrl_hostenv_create; destroy the env before its context
 *     (an env whose context was destroyed first only accepts destroy);
 *   reset / reset_episodes / reset_state / set_time_limit / set_target_velocities /
 *     target_velocities (synchronizes): the host plane's calls of the same names;
 *   step: actions_dev[N][8] (clipped to [-1, 1]) -> one launch, no synchronization;
 *   state_get / state_set: the packed layout above; both synchronize. */
typedef struct ddrl_devenv ddrl_devenv;
int ddrl_devenv_create(ddrl_ctx* ctx, uint64_t seed, float target_velocity, ddrl_devenv** out);
int ddrl_devenv_destroy(ddrl_devenv* env);
int ddrl_devenv_buffers(ddrl_devenv* env, float** obs_dev, float** fw_dev, float** cfrc_dev, float** kin_dev,
                        uint8_t** done_dev);
int ddrl_devenv_reset(ddrl_devenv* env);
int ddrl_devenv_reset_episodes(ddrl_devenv* env);
int ddrl_devenv_reset_state(ddrl_devenv* env);
int ddrl_devenv_set_time_limit(ddrl_devenv* env, int steps);
int ddrl_devenv_set_target_velocities(ddrl_devenv* env, const float* list, int n);
int ddrl_devenv_target_velocities(ddrl_devenv* env, float* out, int n_envs);
/* A fixed target velocity per env: per_env[n_envs] on the host (finite; > 0 with obs_full_dim 44),
 * or NULL to go back to drawing from the list.  With a table set, env e takes per_env[e] at every
 * reset and at every episode restart inside the step kernel.  Synchronizes before the table is
 * replaced; re-keys a captured rollout graph. */
int ddrl_devenv_set_env_target_velocities(ddrl_devenv* env, const float* per_env, int n_envs);
int ddrl_devenv_step(ddrl_devenv* env, const float* actions_dev);
int ddrl_devenv_state_get(ddrl_devenv* env, double* host, size_t n);
int ddrl_devenv_state_set(ddrl_devenv* env, const double* host, size_t n);
/* Uneven ground: the host plane's calls of the same names.  The settings are kernel arguments:
 * they hold for the launches issued after the call (no synchronization), and with terrain on the
 * step runs a second instance of the kernel that evaluates the field under every foot in every
 * substep.  terrain_height takes device pointers (env_index_dev[n], xy_dev[n][2], out_dev[n]) and
 * launches a small kernel on the context's stream; an env index outside [0, n_envs) gives NaN. */
int ddrl_devenv_set_terrain(ddrl_devenv* env, double lo, double hi, double bump_scale, uint32_t generation);
int ddrl_devenv_terrain(ddrl_devenv* env, double* lo, double* hi, double* bump_scale, uint32_t* generation);
int ddrl_devenv_new_terrain(ddrl_devenv* env);
int ddrl_devenv_terrain_height(ddrl_devenv* env, const int32_t* env_index_dev, const double* xy_dev, int n,
                               double* out_dev);
/* A fragment over the device env plane, one in-order chain on the context's stream with no
 * host wait: if reset, ddrl_devenv_reset and observe(env.obs); then for t in [0, T): act(t) ->
 * devenv_step -> reward(t, env.fw, env.cfrc, actions, env.done) -> observe(env.obs); then the
 * bootstrap.  eps_dev[T][N][n_agents][A].  The loop is captured once per (env, eps_dev, env
 * settings: time limit, velocity list or per-env velocity table, and the terrain settings while the ground is not flat --
 * a set_terrain or new_terrain between two fragments re-captures) into a HIP graph and replayed (DDRL_ROLLOUT_GRAPH=0 at context creation issues the
 * launches directly); any model kind. */
int ddrl_rollout_devenv(ddrl_ctx* ctx, ddrl_devenv* env, const float* eps_dev, int reset);

/* Evaluation of the context's policies over whole episodes (evaluation/rollout_episodes.py:26-164):
 * N envs x E episodes each instead of the reference's sequential episodes.  fcnet models only.
 * Reads the weights, coupling table, routing tables and filters; writes no record, done flag,
 * bootstrap value, per-policy filter, Adam state or parameter, and the env-side filter
 * statistics only with filter_update.
 *   eval_begin: allocates / clears the per-env accumulators and the result table [N][E][6]
 *     (rows NaN until written);
 *   eval_act:  one launch: env-side normalization, per-policy filter (read-only), routing,
 *     policy forward and action of every agent from the raw observations obs_dev[N][obs_full_dim];
 *     eps_dev[N][n_agents][A] samples mean + std * eps, NULL takes the mean (RLlib explore=False);
 *     writes the clipped env actions actions_dev[N][8] and, when logits_out_dev (a host array of
 *     n_policies device pointers, entries may be NULL) is given, the logits [C_p][2A] per policy;
 *   eval_step: the env's answer to those actions -- fw_dev[N], cfrc_dev[N][14][6], the actions,
 *     kin_dev[N][9] (ddrl_hostenv_kin's layout), done_dev[N] -- into the fp64 accumulators
 *     {return, power, distance, steps}; a done env below its quota writes its row
 *     {return, steps, distance, power, velocity = distance / steps,
 *      CoT = (power / steps) / (total_mass * velocity)} and every done env restarts;
 *   eval_progress: synchronizes; rows written so far and envs that have filled their quota;
 *   eval_results: the table, n_rows = N * E rows of 6 doubles, env-major. */
typedef struct ddrl_eval_cfg {
  int32_t episodes_per_env;   /* E >= 1 */
  int32_t filter_update;      /* env-side MeanStdFilter keeps pushing during evaluation */
  int32_t ctrl_roll;          /* 2 in the reference (np.roll(ctrl, -2), rollout_episodes.py:146) */
  int32_t reserved;
  double total_mass;          /* 8.78710174560547 (rollout_episodes.py:152) */
} ddrl_eval_cfg;
int ddrl_eval_begin(ddrl_ctx* ctx, const ddrl_eval_cfg* cfg);
int ddrl_eval_act(ddrl_ctx* ctx, const float* obs_dev, const float* eps_dev, float* actions_dev,
                  float* const* logits_out_dev);
int ddrl_eval_step(ddrl_ctx* ctx, const float* fw_dev, const float* cfrc_dev, const float* actions_dev,
                   const float* kin_dev, const uint8_t* done_dev);
int ddrl_eval_progress(ddrl_ctx* ctx, int64_t* episodes_done, int64_t* envs_finished);
int ddrl_eval_results(ddrl_ctx* ctx, double* host, size_t n_rows);
int ddrl_eval_end(ddrl_ctx* ctx);
/* A whole evaluation over the host env plane, loop in C++: reset_episodes, then per step
 * eval_act -> D2H actions -> host step -> H2D (obs, fw, cfrc, kin, done) -> eval_step, until every
 * env has filled its quota (polled every poll_every steps) or max_steps steps ran.  eps_dev: NULL,
 * or eps_steps steps of [N][n_agents][A] noise (the loop then stops at eps_steps at the latest).
 * steps_run (may be NULL): env steps taken. */
int ddrl_eval_hostenv(ddrl_ctx* ctx, ddrl_hostenv* env, const float* eps_dev, int eps_steps, int max_steps,
                      int poll_every, int* steps_run);
/* The same loop over the device env plane, its buffers read in place: reset_episodes, then per
 * step eval_act -> eval_sens (with the mode on) -> devenv_step -> eval_step.  No copies; the only
 * synchronization is the progress poll every poll_every steps. */
int ddrl_eval_devenv(ddrl_ctx* ctx, ddrl_devenv* env, const float* eps_dev, int eps_steps, int max_steps,
                     int poll_every, int* steps_run);
/* Evaluation members: M parameter sets evaluated side by side on one context, n = n_envs / M envs
 * each, in one in-order stream of launches -- a whole sweep of the reference's evaluation scripts
 * (one restored agent per seed / architecture / target velocity cell) as one evaluation.  Member m
 * owns the envs [m n, (m + 1) n) and holds its own parameters (with the "cup" table), env-side
 * filter (running stat, delta stat, constants) and per-policy filter state, in device memory
 * addressed as base + m * stride.  A member computes, bit for bit, what a plain context of n envs
 * holding the same state computes.
 *   eval_members_begin: after eval_begin; 1 <= n_members, n_envs % n_members == 0; allocates the
 *     member storage, all members unloaded.  eval_end (and the next eval_begin) ends the mode;
 *   eval_member_load: stream-ordered device-to-device copies of the context's CURRENT parameters,
 *     env-side filter (n, M, S) and per-policy filter state into the member's slot; its delta
 *     stat starts empty.  Per checkpoint: ddrl_params_set / ddrl_filter_set /
 *     ddrl_policy_filter_set on the context, then eval_member_load(m);
 *   eval_member_filter_get: synchronizes; the member's env-side running stat;
 *   eval_act with the mode on: fails while a member is unloaded ("member k has not been loaded");
 *     otherwise two launches of the filter push for all members (only when filter_update, or once
 *     after a load) and one of the forward, grid (row blocks, policies, members).  It reads and
 *     writes member state only: the context's own parameters and filters are not touched.
 *     obs / eps / actions / logits_out keep their shapes, envs member-major;
 *   eval_step / eval_progress / eval_results / eval_devenv: unchanged (they are per env);
 *   eval_sens_begin and eval_hostenv are refused while the mode is on (sensitivity per member is
 *     not supported; the host env plane has no per-env target velocity). */
int ddrl_eval_members_begin(ddrl_ctx* ctx, int n_members);
int ddrl_eval_member_load(ddrl_ctx* ctx, int member);
int ddrl_eval_member_filter_get(ddrl_ctx* ctx, int member, double* n, double* M, double* S);
/* Input sensitivity ("importance matrix") of the evaluated policies
 * (evaluation/rollout_episodes_compute_gradient.py:59-68, :111-122, :167-168): at every step, every
 * non-constant input feature f of every (env, slot) row is moved by -h_f and +h_f, the 2d perturbed
 * rows go through the policy forward, and mean_plus - mean_minus (clipped action means in the
 * policy's own action order, subtracted in fp32) is added in fp64 into grads[f][j], its magnitude
 * into grads_abs[f][j].  h_f is added to the env-normalized input in fp64, before the per-policy
 * filter and the rounding to fp32.  Constant inputs (the LegID one-hot) are skipped: their rows
 * stay zero.  An env contributes while it is below its episode quota, so the matrices describe
 * the episodes of the result table.  Deterministic (no floating-point atomics): the same calls
 * give the same bits.  Writes no record, filter, Adam state or parameter.
 *   eval_sens_begin: after eval_begin; step_host[p] = obs_dim[p] finite doubles >= 0; allocates and
 *     clears the accumulators.  eval_end (and the next eval_begin) ends the mode;
 *   eval_sens: after eval_act of the same obs_dev and before eval_step; means_out_dev (NULL, or a
 *     host array of n_policies device pointers, entries may be NULL) receives the clipped means
 *     [C_p][2 d][A] of the perturbed rows (row 2f: minus, 2f + 1: plus; NaN for constant inputs);
 *   eval_sens_results: synchronizes, sums over rows in a fixed order; grads / grads_abs are
 *     [obs_dim][A] doubles on the host, rows the (env, slot) rows accumulated over all steps.
 * With the mode on, ddrl_eval_hostenv issues eval_sens after every eval_act. */
int ddrl_eval_sens_begin(ddrl_ctx* ctx, const double* const* step_host);
int ddrl_eval_sens(ddrl_ctx* ctx, const float* obs_dev, float* const* means_out_dev);
int ddrl_eval_sens_results(ddrl_ctx* ctx, int policy, double* grads, double* grads_abs, int64_t* rows);

/* Postprocessing: GAE over the fragment for every policy + advantage standardization
 * statistics (a11/a12). */
int ddrl_gae(ddrl_ctx* ctx);
/* fp64 {sum adv, sum adv^2, count} of policy pid from the last ddrl_gae, for a cross-rank
 * StandardizeFields (the global {mean, max(1e-4, std)} goes back through adv_norm_set). */
int ddrl_adv_sums_get(ddrl_ctx* ctx, int pid, double* host3);

/* Episode accounting of the training rollout: the episodes that finished in the fragment, as
 * RLlib 1.0 counts them (3p evaluation/episode.py MultiAgentEpisode._add_agent_rewards, summarized
 * by 3p evaluation/metrics.py summarize_episodes into episode_reward_mean / episode_len_mean /
 * policy_reward_mean -- column 2 against column 6 of Tune's progress.csv is every learning curve
 * of the reference: visualization/visualize_learning_over_time.py:49-53,
 * stats/compare_learning_performance_atEnd.py:104-108).  Per env step, for every agent in agent
 * order, agent_total[j] += r and total += r in fp64, r the fp32 reward of the agent's record
 * (what the learner trains on); length counts env steps and the step that raises done belongs to
 * the episode it ends.  Only done flags end an episode: an env reset behind the rollout
 * (update_environment_after_epoch, quantruped_adaptor_multi_environment.py:97-122) does not.
 * The running sums of every env persist in the context across fragments (allocated by the first
 * call here).  Deterministic: row positions come from counts and a scan, no atomics.  Writes no
 * record, done flag, bootstrap value, filter, Adam state or parameter.
 *   episodes_collect: after the fragment's last ddrl_reward: counts, scans, sizes the table, walks
 *     the fragment forward.  Synchronizes once.  A fragment is collected at most once (the walk
 *     advances the in-flight state): a second collect fails until ddrl_reward / ddrl_reward_range,
 *     ddrl_rollout_hostenv, a ddrl_rollout_fragment launch or ddrl_records_set brought new rewards;
 *   episodes_rows: the rows of the last collect, n_rows == n_finished, 8 doubles each
 *     {t, env, length, total, agent_0 .. agent_3} (agents the env does not have: NaN), in
 *     ascending (t, env) order;
 *   episodes_inflight: the state of every env's running episode [n_envs][6] =
 *     {total, agent_0 .. agent_3 (0 for agents the env does not have), length} (tests, diagnostics);
 *   episodes_reset: forget the in-flight episodes (a caller that resets envs and wants them
 *     dropped). */
int ddrl_episodes_collect(ddrl_ctx* ctx, int64_t* n_finished);
int ddrl_episodes_rows(ddrl_ctx* ctx, double* host, size_t n_rows);
int ddrl_episodes_inflight(ddrl_ctx* ctx, double* host, size_t n_envs);
int ddrl_episodes_reset(ddrl_ctx* ctx);

/* PPO update of policy pid_mask bits (a13-a17).  Per policy p (bit p set):
 *   shuffle_dev[p] : int32[R_p] row permutation (SampleBatch.shuffle)
 *   perm_dev[p]    : int32[num_sgd_iter][nb_p] minibatch-slot permutation per epoch,
 *                    nb_p = max(1, R_p / sgd_minibatch_size)
 *   kl_coeff[p]    : current KL coefficient
 * max_steps < 0 runs the whole schedule; >= 0 runs only the first max_steps minibatches.
 * All policies in the mask run concurrently (one persistent workgroup each).
 * Row i of step (e, b) is shuffle[perm[e][b] * sgd_minibatch_size + i]; rows past
 * nb * sgd_minibatch_size are left out; a train batch of fewer rows than one minibatch is refused.
 * sgd_minibatch_size = 256 (fcnet models): the same schedule, statistics and rollback through
 * the 256-row kernels, each of a branch's two workgroups on 128 rows.  It needs the row split
 * (DDRL_UPDATE_SPLIT=1 is refused at ddrl_ctx_create).  Of the data-parallel entry points,
 * ddrl_ppo_grad / ddrl_ppo_apply and ddrl_ppo_update_ddp work with rows_per_rank <= 128 (the
 * gradient is scaled by 1 / 256, so the split over two or more ranks sums to the 256-row
 * gradient); a whole 256-row minibatch per rank ("local" mode) and peer mode (ddrl_peer_attach)
 * are refused. */
int ddrl_ppo_update(ddrl_ctx* ctx, int pid_mask, const int32_t* const* shuffle_dev,
                    const int32_t* const* perm_dev, const float* kl_coeff, int max_steps);
/* The same update resumed at minibatch step step0 of the schedule (step0 = e * nb + b), from the
 * weights, Adam state and beta powers the context holds (e.g. restored from a mid-update
 * checkpoint): bit-identical to steps step0 .. of one uninterrupted ddrl_ppo_update (round 6; the
 * fused exchange's tag bits follow the schedule step).  Learner statistics land in rows step0 ..;
 * max_steps counts from step0.  ddrl_ppo_update is ddrl_ppo_update_from(…, 0, max_steps). */
int ddrl_ppo_update_from(ddrl_ctx* ctx, int pid_mask, const int32_t* const* shuffle_dev,
                         const int32_t* const* perm_dev, const float* kl_coeff, int step0, int max_steps);
/* Per-minibatch learner stats of the last update: n_steps x 8 floats
 * {total_loss, policy_loss, vf_loss, kl, entropy, vf_explained_var, grad_gnorm, clip_scale}. */
int ddrl_ppo_stats(ddrl_ctx* ctx, int pid, float* host, size_t n_steps);
/* Rows [first, first + n_steps) of the same statistics: RLlib's learner stats and update_kl
 * (3p ppo.py update_kl, on the last epoch's mean KL) need only the last epoch's nb rows. */
int ddrl_ppo_stats_range(ddrl_ctx* ctx, int pid, size_t first, size_t n_steps, float* host);

/* Group update: the fused PPO updates of M contexts of one shape -- e.g. the seeds of one
 * experiment -- in one launch.  One run's chains cannot be widened (four sequential chains on 16
 * CUs), several runs' chains are independent: chain m * n_policies + p (policy p of member m)
 * runs on blocks 32 (c >> 3) + 8 j + (c & 7) of its launch, c its index in the launch, j = 0 .. 3 (policy / value branch x
 * row half), so the four workgroups of a chain share an XCD as a context's do.  Every member stays
 * a full, ordinary context (its own records, schedule, weights, Adam state, KL coefficients), and
 * each chain computes, bit for bit, what ddrl_ppo_update on its context alone computes.  fcnet
 * models, sgd_minibatch_size 128, the row split and the default exchange protocol only.
 *   create: members[n_members], all on one device and one stream (the group enqueues on it).
 *     Refuses, naming the member and the reason: no member, a null or repeated context, another
 *     device or stream, a ddrl_cfg that differs from member 0's in anything the update reads, a
 *     GraphNet member, sgd_minibatch_size 256, DDRL_UPDATE_SPLIT=1, the atomic protocol, an attached
 *     peer.  max_chains_per_launch: 0 = the device's cap, 8 * floor((CUs / 8) / 4) chains (all
 *     workgroups of a launch spin on partners and must be resident, one per CU: 64 chains on an
 *     MI355X); a group with more chains, or a smaller value here, runs as several launches in
 *     stream order, whole members per launch, with the same results.  The group owns the argument
 *     table (device, filled from a pinned host buffer), the exchange arenas, its error word, its
 *     launch epoch and the per-block XCC record.  Destroy the group before its members.
 *   run: ddrl_ppo_update for every policy of every member from schedule step 0: shuffle_dev /
 *     perm_dev / kl_coeff hold n_members * n_policies entries, member-major; max_steps is common.
 *     Takes each member's snapshot; ddrl_ppo_stats* on a member afterwards work unchanged.
 *     Asynchronous; one run at a time (finish it before the next).
 *   finish: synchronizes and checks.  On failure (an exchange abandoned after 3 s -- e.g. a grid
 *     that was not resident -- or a failed launch) every member's snapshot is restored and the
 *     message says so.  When a chain's four blocks ran on different XCDs the message names the
 *     placement check and the group refuses further runs: update the members one by one.
 *   plan: pure host function (no GPU): launch_of_member[n_members] and
 *     first_block_of_chain[n_members * n_policies] (the chain's block 8 j apart, in its launch's
 *     grid) for launches of at most max_chains chains.  A launch of n chains has
 *     32 (ceil(n / 8) - 1) + 24 + (n - 8 (ceil(n / 8) - 1)) blocks.
 *   placement: after finish; the XCC id of every block of the last run, the launches' grids in
 *     launch order; n_blocks >= their sum, the entries past it are set to -1 (-1 too for a run
 *     that has not finished yet). */
typedef struct ddrl_update_group ddrl_update_group;
int ddrl_update_group_create(ddrl_ctx* const* members, int n_members, int max_chains_per_launch,
                             ddrl_update_group** out);
int ddrl_update_group_run(ddrl_update_group* group, const int32_t* const* shuffle_dev,
                          const int32_t* const* perm_dev, const float* kl_coeff, int max_steps);
int ddrl_update_group_finish(ddrl_update_group* group);
int ddrl_update_group_plan(int n_members, int n_policies, int max_chains, int32_t* launch_of_member,
                           int32_t* first_block_of_chain);
int ddrl_update_group_placement(ddrl_update_group* group, int32_t* xcc, int n_blocks);
int ddrl_update_group_destroy(ddrl_update_group* group);
/* stats_range: ddrl_ppo_stats_range(first, n_steps) of every policy of every member after a finished
 * run, host[n_members][n_policies][n_steps][8]: every copy is enqueued, then one synchronize.  The
 * per-context call's refusals (a null buffer, a range past the schedule's rows, a set error word),
 * and a run that has not been finished. */
int ddrl_update_group_stats_range(ddrl_update_group* group, size_t first, size_t n_steps, float* host);

/* Group rollout (rollout_group.hip): the device-plane fragments of n_members same-shaped contexts
 * as ONE in-order chain of launches, the member in the grid's z.  Member m is the context
 * members[m] with its own device env plane envs[m] (created on that context); every member stays
 * a full, ordinary context and env, and the chain leaves on each, bit for bit, what
 * ddrl_rollout_devenv(members[m], envs[m], eps_dev[m], reset) alone leaves: records, last values,
 * both filters, the env state and the host-side notes, so ddrl_gae, ddrl_episodes_collect and the
 * update (solo or group) follow on a member unchanged.  fcnet models only.
 *   create: members[n_members] and envs[n_members], all on one device and one stream (the group
 *     enqueues on it).  Refuses, naming the member and the reason: no member, a null or repeated
 *     context or env, a GraphNet member, a ddrl_cfg that differs from member 0's in anything the
 *     rollout kernels read (n_envs and frag_len included), an env bound to another context than
 *     its member, another device or stream, members whose terrain on / off or target-velocity
 *     mode (list draws / per-env table) differ -- the step kernel's instance is one per launch.
 *     The group owns the member table (device, filled from a pinned host buffer).  Destroy the
 *     group before its members and their envs.
 *   run: eps_dev[n_members], each [T][N][n_agents][A] in device memory.  If reset, every member's
 *     ddrl_devenv_reset and observe first.  Then for t in [0, T): act(t) -> env step -> reward(t)
 *     -> filter push -> (per-policy filter) -> observe, and the bootstrap: 6 to 8 launches per
 *     step for the whole group.  The member table is rebuilt from the members' current state at
 *     every run, so a time limit, target velocities or terrain set between runs hold.  The
 *     launches are issued directly (no graph); no host synchronization except, from the second
 *     run on, a wait for the previous run's table copy.  Refuses what create refuses of a
 *     member's env, stream, terrain and velocity mode, and a null noise buffer; after a refusal
 *     destroy remains valid. */
typedef struct ddrl_rollout_group ddrl_rollout_group;
int ddrl_rollout_group_create(ddrl_ctx* const* members, ddrl_devenv* const* envs, int n_members,
                              ddrl_rollout_group** out);
int ddrl_rollout_group_run(ddrl_rollout_group* group, const float* const* eps_dev, int reset);
int ddrl_rollout_group_destroy(ddrl_rollout_group* group);

/* Group finish (finish_group.hip): what lies between a fragment's last env step and the update --
 * ddrl_gae and ddrl_episodes_collect -- for n_members same-shaped contexts as ONE in-order chain of
 * launches, the member in the grid's z, with one host synchronize for the group where the plain
 * calls have one per member.  Only the records are read, so the fragment may come from any env
 * plane and any model kind (GraphNet included).  Every member stays a full, ordinary context and
 * is left, bit for bit, as ddrl_gae + ddrl_episodes_collect leave it (adv / vt columns, adv_norm,
 * the GAE totals, the episode table, the in-flight state and the host-side notes), so
 * ddrl_episodes_rows, ddrl_episodes_inflight, ddrl_adv_sums_get, ddrl_adv_norm_get, the "collected
 * once" refusal and a following update (solo or group) behave unchanged.
 *   create: members[n_members] (at most 65535), all on one device and one stream (the group
 *     enqueues on it).  Refuses, naming the member and the reason: no member, a null or repeated
 *     context, another device or stream, and "finish group: member m differs from member 0 in
 *     <field>" for the first of n_envs, frag_len, n_agents, n_policies, agent_policy, the record
 *     layout, gamma, lambda_ that differs.  The group owns the member table (device, filled from a
 *     pinned host buffer) and the totals array.  Destroy the group before its members.
 *   run: the GAE scan and its finalize, the episode count and scan, one copy of the members' totals
 *     and the synchronize, the plain collect's count check and table growth (max(total, 2 * cap))
 *     per member on the host, the walk.  n_finished[n_members]: rows per member.  The member table
 *     is rebuilt at every run from the members' current state.  If any member has been collected
 *     this fragment, the whole run is refused before anything is launched.
 *   rows: ddrl_episodes_rows of every member, host[m] holding n_rows[m] rows of 8 doubles, with one
 *     synchronize; refuses an n_rows[m] that differs from member m's last count. */
typedef struct ddrl_finish_group ddrl_finish_group;
int ddrl_finish_group_create(ddrl_ctx* const* members, int n_members, ddrl_finish_group** out);
int ddrl_finish_group_run(ddrl_finish_group* group, int64_t* n_finished);
int ddrl_finish_group_rows(ddrl_finish_group* group, double* const* host, const int64_t* n_rows);
int ddrl_finish_group_destroy(ddrl_finish_group* group);

/* Device randomness (rng.hip): the exploration noise of a fragment and the minibatch schedules of an
 * update drawn on the device by a counter-based generator, Philox4x32-10 (csrc/philox.h; the exact
 * counter and key layout: DESIGN.md section 3, "Device randomness").  A context has two streams,
 * each a 64-bit seed and a 64-bit position: a draw is a pure function of (seed, position, element),
 * so it is the same solo, as a group member or in chunks, and the whole state is two integers.
 * Opt-in: a context whose streams are never seeded behaves as before.  Any model kind (only shapes
 * are read).  All calls are asynchronous on the context's stream.
 *   rng_seed: the stream's seed; its position := 0.  rng_state_get / rng_state_set: (seed, position),
 *     e.g. for a checkpoint; set also rewinds.  get on an unseeded stream is refused.
 *   noise_fill: eps_dev[n_steps][N][n_agents][A] (16-byte aligned) standard normals for the absolute
 *     steps [position, position + n_steps) of the noise stream; position += n_steps.  The value at
 *     (step, env, agent, action) does not depend on N, n_steps or the launch geometry.  Needs
 *     n_agents * A to be a multiple of 4 (it is 8 in every registered env).
 *   schedule_fill: for every policy p in pid_mask, shuffle_dev[p] : int32[R_p] and perm_dev[p] :
 *     int32[num_sgd_iter][nb_p] as ddrl_ppo_update takes them, each a keyed bijection of [0, n) (a
 *     balanced Feistel network with Philox round functions, cycle-walked; no sort).  The key is
 *     (schedule seed, draw index = position, policy, array); position += 1 per call.
 *   noise_fill_group / schedule_fill_group: the same for n_members contexts of one shape in ONE
 *     launch, the member in the grid's z and its operands in a device table filled from a pinned
 *     host buffer (owned by members[0]); eps_dev[m] is member m's buffer, shuffle_dev / perm_dev
 *     hold n_members * n_policies entries, member-major, and every policy is filled.  Each member
 *     is left exactly as by its solo call: the buffers and the advanced position.  All members on
 *     one device and one stream; a null or repeated member, another device, stream or shape is
 *     refused naming the member.
 * Refused with a message: an unseeded stream, null buffers, n_steps < 1, a policy bit outside the
 * context, a misaligned noise buffer. */
enum { DDRL_RNG_NOISE = 0, DDRL_RNG_SCHEDULE = 1 };
int ddrl_rng_seed(ddrl_ctx* ctx, int stream, uint64_t seed);
int ddrl_rng_state_get(ddrl_ctx* ctx, int stream, uint64_t* seed, uint64_t* position);
int ddrl_rng_state_set(ddrl_ctx* ctx, int stream, uint64_t seed, uint64_t position);
int ddrl_noise_fill(ddrl_ctx* ctx, int n_steps, float* eps_dev);
int ddrl_schedule_fill(ddrl_ctx* ctx, int pid_mask, int32_t* const* shuffle_dev, int32_t* const* perm_dev);
int ddrl_noise_fill_group(ddrl_ctx* const* members, int n_members, int n_steps, float* const* eps_dev);
int ddrl_schedule_fill_group(ddrl_ctx* const* members, int n_members, int32_t* const* shuffle_dev,
                             int32_t* const* perm_dev);

/* Data-parallel (shared policy) primitives: gradient of (1/minibatch) * sum over the
 * given rows -> grad_dev[n_params]; after the caller's all-reduce (RCCL), apply clip +
 * Adam.  rows_dev holds n_rows (<= 128) record indices.  stats_step >= 0 also writes this
 * rank's loss statistics of the rows (means over n_rows) into stats row stats_step. */
int ddrl_ppo_grad(ddrl_ctx* ctx, int pid, const int32_t* rows_dev, int n_rows,
                  float kl_coeff, float* grad_dev, int stats_step);
int ddrl_ppo_apply(ddrl_ctx* ctx, int pid, const float* grad_dev);

/* RCCL communicator of a data-parallel learner (SURVEY 8(b) "ddrl_comm_init"; replaces the
 * GPU-tower gradient averaging of RLlib's TrainTFMultiGPU, 3p execution/train_ops.py, which
 * the reference sizes with ray.init(num_gpus=...) at train_experiment_1_architecture_on_flat.py:94
 * and the commented config['num_gpus'] at :103-106).  Rank 0 makes
 * the unique id (DDRL_COMM_ID_BYTES bytes, handed to the other ranks by the caller, e.g. a
 * torch.distributed broadcast), every rank joins with its rank; one communicator per context,
 * on the context's device.  comm_allreduce sums n floats in place on the context's stream. */
#define DDRL_COMM_ID_BYTES 128
int ddrl_comm_unique_id(void* id_out, size_t n);
int ddrl_comm_init(ddrl_ctx* ctx, const void* id, int rank, int nranks);
int ddrl_comm_allreduce(ddrl_ctx* ctx, float* buf_dev, size_t n);
/* The data-parallel minibatch SGD of policy pid, enqueued from C++ on the context's stream
 * (per step: gradient of this rank's rows -> RCCL all-reduce -> clip + Adam), the per-step
 * loop of ddrl_amd/ddp.py DataParallelLearner.learn without a host round trip per call.
 *   shuffle_dev: this rank's row permutation; perm_host[n_epochs][nb]: minibatch slots;
 *   rows_per_rank: 128 / ranks ("split") or 128 ("local"); grad_scale: 1 or 1 / ranks.
 * Learner statistics of the last epoch land in ddrl_ppo_stats rows 0 .. nb - 1.
 * The records of each run of up to 1,024 steps are gathered on the device into one chunk
 * (allocated by the first call: min(1024, steps) x rows_per_rank x record stride floats) before
 * that run's gradient launches; perm_host is copied to the device once per call. */
int ddrl_ppo_update_ddp(ddrl_ctx* ctx, int pid, const int32_t* shuffle_dev, const int32_t* perm_host,
                        int n_epochs, int nb, int rows_per_rank, float kl_coeff, float grad_scale);

/* Peer mode (round 5): the shared-policy minibatch SGD of two ranks as ONE
 * fused persistent update split across the ranks' contexts -- the reference's 128-row minibatch
 * ("split" semantics; train_shared_policy_architecture_on_flat.py:48,79 via RLlib's
 * TrainTFMultiGPU) with rank r's 64 rows of every minibatch in rank r's fused launch, which swaps
 * its partial gradients with the peer launch every step through shared outboxes (LSB-tagged
 * quads, system-scope stores and loads; no collective, no per-step launch), then runs the same
 * clip + Adam:
 * both ranks' weights stay bit-identical to each other and to one fused launch over the union
 * batch.  fcnet models, row split on (the default), two ranks, sgd_minibatch_size 128 (a 256
 * context is refused at ddrl_peer_attach).
 *   ddrl_peer_alloc: rank 0 allocates the outboxes (fine-grained device memory, cleared) and,
 *     with ipc_handle_out, exports them (DDRL_PEER_HANDLE_BYTES, hipIpcGetMemHandle);
 *   ddrl_peer_open: rank 1 maps rank 0's outboxes from that handle (another process);
 *   ddrl_peer_attach: both ranks, before their first peer update (a context in the same
 *     process passes rank 0's pointer directly); resets the launch tags; rank 0's attach also
 *     clears the outboxes, so rank 1 attaches after it (and after a failed update both re-attach);
 *     it reserves the buffers of num_sgd_iter epochs of R / 64 slots (a larger schedule grows
 *     them, which waits for the whole device: a stall for a peer context of the same process);
 *   ddrl_ppo_update_peer: shuffle_dev = this rank's nb * 64 row indices (minibatch slot b owns
 *     entries [64 b, 64 b + 64)), perm_dev[n_epochs][nb] = the slots, the same on both ranks.
 *     Both ranks must issue the same sequence of peer updates, and each launch needs its peer's
 *     launch to run concurrently (a wait abandoned after 3 s raises, with the snapshot restored).
 *     A failed peer update detaches the context: the next ddrl_ppo_update_peer is refused ("no
 *     peer") until both ranks have called ddrl_peer_attach again, which clears the outboxes. */
#define DDRL_PEER_HANDLE_BYTES 64
int ddrl_peer_alloc(ddrl_ctx* ctx, void** gx_out, void* ipc_handle_out);
int ddrl_peer_open(ddrl_ctx* ctx, const void* ipc_handle, void** gx_out);
int ddrl_peer_attach(ddrl_ctx* ctx, void* gx, int rank, int nranks);
int ddrl_ppo_update_peer(ddrl_ctx* ctx, int pid, const int32_t* shuffle_dev, const int32_t* perm_dev,
                         int n_epochs, int nb, float kl_coeff, int max_steps);

/* The GraphNet context's minibatch step as it runs now: *on = 1 for the one-launch step (the
 * gradient launch reduces over its tiles and runs clip + Adam in its tail), 0 for the three-launch
 * step (k_gnn + k_gnn_reduce + k_gnn_adam) -- DDRL_GNN_TAIL=0, an occupancy or owner-list refusal,
 * or a fallback after a failed one-launch step -- or before the first 128-row step has built
 * the owner lists; 0 for an fcnet context. */
int ddrl_gnn_one_launch(ddrl_ctx* ctx, int* on);

/* Model forward (ModelV2.forward + value_function) on arbitrary rows:
 * obs_dev[n][d] (ffn; + node_dev[n] = leg index with leg_coupling) or X_dev[n][4][23] +
 * node_dev[n] (gnn). */
int ddrl_policy_forward(ddrl_ctx* ctx, int pid, const float* obs_dev, const int32_t* node_dev,
                        int n, float* logits_dev, float* values_dev);

/* Training-row buffers (SampleBatch columns) of policy pid, [T*C][row_stride] floats:
 * read back for inspection, or loaded from an external batch (e.g. a replayed SampleBatch). */
int ddrl_records_get(ddrl_ctx* ctx, int pid, float* host, size_t n_floats);
int ddrl_records_set(ddrl_ctx* ctx, int pid, const float* host, size_t n_floats);
/* Advantage standardization constants {mean, max(1e-4, std)} of policy pid. */
int ddrl_adv_norm_get(ddrl_ctx* ctx, int pid, float* host2);
int ddrl_adv_norm_set(ddrl_ctx* ctx, int pid, float mean, float denom);
/* Bootstrap values V(s_T) of policy pid, C floats (set: for a replayed batch). */
int ddrl_last_values_get(ddrl_ctx* ctx, int pid, float* host, size_t n);
int ddrl_last_values_set(ddrl_ctx* ctx, int pid, const float* host, size_t n);
/* Episode-end flags of the fragment, [T][N] bytes (normally written by ddrl_reward). */
int ddrl_done_set(ddrl_ctx* ctx, const uint8_t* host, size_t n);

/* Direct device pointers (for zero-copy inspection and collectives). */
int ddrl_device_buffers(ddrl_ctx* ctx, int pid, void** records, void** last_v, void** params,
                        void** adv_norm);

#ifdef __cplusplus
}
#endif
#endif
