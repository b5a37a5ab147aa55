// Host-side launch wrappers shared between the kernel translation units and the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DDRL_MAXP 4       // policies per context
#define DDRL_MAXAG 4      // agents per env
#define DDRL_MAXD 48      // per-agent observation width
#define DDRL_MAXFULL 48   // full observation width (43 / 44)
#ifndef DDRL_MB
#define DDRL_MB 128       // sgd_minibatch_size of the update kernels (256: ppo_ffn_mb256.hip defines it first)
#endif

// Record (one training row) layout, in floats.  Rows are time-major:
//   row = t * C + c,  c = env * k + slot  (k agents of this policy per env).
struct RecLayout {
  int stride;      // floats per row (multiple of 4)
  int obs, act, logit, logp, vf, adv, vt, rew;
  int cid;         // leg index of the row ("cup" model), -1 when the model has no coupling
};

// Per-policy routing tables for the observe / act / reward kernels.
struct PolicyRoute {
  int k;                    // agents of this policy per env
  int d;                    // obs width per row (GNN: 19 features per node)
  int agent[DDRL_MAXAG];    // agent id of each slot
  int obs_index[DDRL_MAXAG][DDRL_MAXD];
  int act_index[DDRL_MAXAG][8];
  int act_neg[DDRL_MAXAG];         // bit j: negate action j in the env vector (LegTransforms)
};

struct RouteArgs {
  int P, N, A, full_dim, n_agents, model;   // model: 0 ffn, 1 gnn
  int e0;                                   // env range [e0, e0 + N) of a ranged observe (host env plane)
  PolicyRoute pol[DDRL_MAXP];
  float leg_angle[4];
};

// launch geometry of the per-row kernels: the most rows (n_envs * k) and the widest observation
// of the routed policies
struct RowGeom { int rows, d; };
inline RowGeom row_geom(const RouteArgs& ra, int n_envs) {
  RowGeom g{0, 0};
  for (int p = 0; p < ra.P; ++p) {
    g.rows = ra.pol[p].k * n_envs > g.rows ? ra.pol[p].k * n_envs : g.rows;
    g.d = ra.pol[p].d > g.d ? ra.pol[p].d : g.d;
  }
  return g;
}

// ---- filter / observe (rollout.hip) ----
// dn / dM / dS: a second running stat of the pushes since the last cross-rank filter sync
// part: filter_part_doubles(N, D) doubles of per-chunk (mean, M2) scratch
#define FP_ROWS 256   // rows per filter chunk: one per thread
void launch_filter_push(hipStream_t s, const float* obs, int N, int D, double* n_run, double* M,
                        double* S, double* normc, int update, int enabled, double* dn, double* dM,
                        double* dS, double* part);
size_t filter_part_doubles(int N, int D);
// the batch count of the env-side filter push, added by the observe kernel
struct FilterCount { double* n_run; double* dn; int count; };
// pf: per-policy RLlib MeanStdFilter state (PF_* layout, nullptr when disabled)
void launch_observe_ffn(hipStream_t s, const RouteArgs& ra, const float* obs, const double* normc,
                        float clip, float* const* stage, const double* pf, const FilterCount& fc);
// per-policy filter: statistics of the env-normalized observation columns, then the
// RunningStat update + normalization constants of every policy column
#define PF_N 0
#define PF_M 1
#define PF_S (PF_M + DDRL_MAXD)
#define PF_DN (PF_S + DDRL_MAXD)
#define PF_DM (PF_DN + 1)
#define PF_DS (PF_DM + DDRL_MAXD)
#define PF_NORMC (PF_DS + DDRL_MAXD)
#define PF_STRIDE (PF_NORMC + 2 * DDRL_MAXD)
void launch_policy_filter(hipStream_t s, const RouteArgs& ra, const float* obs, const double* normc, float clip,
                          double* zs, double* pf, int update);
void launch_observe_gnn(hipStream_t s, const RouteArgs& ra, const float* obs, const double* normc,
                        float clip, float* stage_x /*[N][4][23]*/, const FilterCount& fc);

// ---- act (rollout forward + sample) ----
struct ActArgs {
  const float* theta[DDRL_MAXP];
  const float* stage[DDRL_MAXP];   // [C][d] (ffn) or [N][4][23] (gnn)
  float* rec[DDRL_MAXP];           // base of the record buffer of this policy
  const float* cup[DDRL_MAXP];     // "cup" leg-coupling table [4][A] (nullptr: none)
  float* last_v[DDRL_MAXP];
  RecLayout lay[DDRL_MAXP];
  int C[DDRL_MAXP];
  int t;                           // time index (record row block)
  const float* eps;                // [N][n_agents][A]
  float* actions;                  // [N][8]
  int bootstrap;                   // 1: only value -> last_v
  int e0, e1;                      // env range of this call ([0, N) for a whole step)
};
void launch_act_ffn(hipStream_t s, const RouteArgs& ra, const ActArgs& aa);
void launch_act_gnn(hipStream_t s, const RouteArgs& ra, const ActArgs& aa, int layer);

// ---- reward (a8) ----
struct RewardArgs {
  int P, N, n_agents, mode;         // mode: 0 per-leg, 1 global, 2 norm_reward
  float ctrl_w, contact_w;
  int policy_of_agent[DDRL_MAXAG];
  int slot_of_agent[DDRL_MAXAG];
  int k[DDRL_MAXP];
  int act_index[DDRL_MAXAG][8];
  int n_act[DDRL_MAXAG];
  int n_contact[DDRL_MAXAG];
  int contact_index[DDRL_MAXAG][14];
  float contact_weight[DDRL_MAXAG][14];
  float* rec[DDRL_MAXP];
  RecLayout lay[DDRL_MAXP];
  int t;
  int e0, n;                        // env range [e0, e0 + n) of this call (N: all envs)
};
void launch_reward(hipStream_t s, const RewardArgs& ra, const float* fw, const float* cfrc,
                   const float* actions, const uint8_t* done, uint8_t* done_tn);

// ---- evaluation (eval.hip): fused observe + forward + action, episode statistics ----
// what the evaluation kernels read to turn a raw observation into a policy's action means
struct PolicyInputArgs {
  const float* theta[DDRL_MAXP];
  const float* cup[DDRL_MAXP];     // "cup" leg-coupling table [4][A] (nullptr: none)
  const float* obs;                // raw observations [N][full_dim]
  const double* normc;             // env-side filter constants (mean, std + 1e-8) per column
  const double* pf;                // per-policy filter state (PF_* layout) or nullptr
  float clip;
};
struct EvalActArgs {
  PolicyInputArgs in;
  float* logits_out[DDRL_MAXP];    // optional [C_p][2A] logits of this step (nullptr: not written)
  const float* eps;                // [N][n_agents][A]; nullptr: deterministic (the mean)
  float* actions;                  // [N][8]
  FilterCount fc;                  // batch count of this step's env-side filter push (0: none)
};
void launch_eval_act(hipStream_t s, const RouteArgs& ra, const EvalActArgs& ea);
struct EvalAccumArgs {
  double* acc;                     // [N][4]: return, power, distance, steps of the running episode
  int32_t* ep_count;               // [N] episodes recorded per env
  double* table;                   // [N][E][6]: return, steps, distance, power, velocity, CoT
  unsigned long long* counters;    // [2]: episodes recorded, envs that filled their quota
  int E, ctrl_roll;
  double total_mass;
};
// ra: the reward tables of launch_reward (rec / lay / t unused); kin[N][9] = {dx, joint qvel[8]}
void launch_eval_accum(hipStream_t s, const RewardArgs& ra, const EvalAccumArgs& ev, const float* fw,
                       const float* cfrc, const float* actions, const float* kin, const uint8_t* done);

// ---- evaluation members (eval_members.hip): M parameter sets side by side, n envs each ----
// Member m owns the envs [m n, (m + 1) n).  Its state is addressed as base + m * stride, the
// strides by value in the argument block (no per-member pointer table anywhere).
// The env-side filter of a member, one block of FM_STRIDE doubles: running stat (n, M, S), the
// delta stat (pushes since the load) and the normalization constants (mean, std + 1e-8) per column
#define FM_N 0
#define FM_M 1
#define FM_S (FM_M + DDRL_MAXFULL)
#define FM_DN (FM_S + DDRL_MAXFULL)
#define FM_DM (FM_DN + 1)
#define FM_DS (FM_DM + DDRL_MAXFULL)
#define FM_NORMC (FM_DS + DDRL_MAXFULL)
#define FM_STRIDE (FM_NORMC + 2 * DDRL_MAXFULL)
struct EvalMembersArgs {
  const float* theta[DDRL_MAXP];   // member 0's flat parameters of each policy (the cup table included)
  size_t theta_stride[DDRL_MAXP];  // floats from one member's parameters to the next
  int cup_off[DDRL_MAXP];          // offset of the "cup" table [4][A] in the parameters (< 0: none)
  const float* obs;                // raw observations [M n][full_dim]
  double* filt;                    // [M][FM_STRIDE]; the act kernel advances the counts
  const double* pf;                // [M][P][PF_STRIDE] per-policy filter state, or nullptr
  size_t pf_stride;                // doubles per member
  float clip;
  float* logits_out[DDRL_MAXP];    // optional [M n k_p][2A], member-major
  const float* eps;                // [M n][n_agents][A] or nullptr
  float* actions;                  // [M n][8]
};
// ra.N = n, the envs of ONE member; grid (ceil(n k_max / 64), P, M).  count: the batch count of this
// step's env-side filter push (0: none), added to every member's counts as FilterCount's is
void launch_eval_act_members(hipStream_t s, const RouteArgs& ra, const EvalMembersArgs& ma, int n_members, int count);
// launch_filter_push with a member index in the grid: chunks counted from the member's first env,
// merged in order; the count of a pushed batch is left to launch_eval_act_members behind it.
// part: n_members * filter_part_doubles(n, D) doubles
void launch_filter_push_members(hipStream_t s, const float* obs, int n, int D, int n_members, double* filt,
                                int update, int enabled, double* part);

// ---- input sensitivity of the evaluated policies (eval_sens.hip) ----
struct EvalSensArgs {
  PolicyInputArgs in;              // normc: as the step's ddrl_eval_act read them
  float* means_out[DDRL_MAXP];     // optional [C_p][2 d][A] clipped means of the perturbed rows (nullptr)
  double* acc[DDRL_MAXP];          // [C_p][2][d][A]: per base row, sum of (plus - minus) and of its magnitude
  long long* rowcnt[DDRL_MAXP];    // [C_p] steps accumulated per base row
  const double* step;              // [P][DDRL_MAXD] perturbation h_f of the env-normalized input
  const int32_t* ep_count;         // [N] episodes recorded per env (the quota gate)
  int E;
};
// grid_cap: most workgroups per policy; a workgroup loops over base rows when there are more
void launch_eval_sens(hipStream_t s, const RouteArgs& ra, const EvalSensArgs& sa, int grid_cap);
// out[n] = sum over the C rows, in row order, of acc[C][n]; rows[0] = sum of rowcnt[C]
void launch_sens_reduce(hipStream_t s, const double* acc, const long long* rowcnt, int C, int n, double* out,
                        long long* rows);

// ---- GAE + standardization statistics ----
struct GaeArgs {
  float* rec; RecLayout lay; int C, T, N, k;
  const float* last_v; const uint8_t* done_tn;
  double gamma, lambda_;
  // totals {sum adv, sum adv^2, count} at [2 * ceil(C / 256)], per-wave partial sums
  // [ceil(C / 64)][2] from gae_wave_base(C); gae_partials_len(C) doubles in all
  double* partials;
  float* adv_norm;    // [2]: mean, max(1e-4, std)
};
__host__ __device__ inline int gae_wave_base(int C) { return 2 * ((C + 255) / 256) + 4; }
__host__ __device__ inline int gae_partials_len(int C) { return gae_wave_base(C) + 2 * ((C + 63) / 64); }
struct GaeBatch { GaeArgs g[DDRL_MAXP]; int P; };
void launch_gae(hipStream_t s, const GaeBatch& gb);   // every policy of the context, one launch

// ---- episode accounting of the training rollout (episodes.hip) ----
struct EpArgs {
  const float* rec[DDRL_MAXP]; RecLayout lay[DDRL_MAXP]; int k[DDRL_MAXP];
  int policy_of_agent[DDRL_MAXAG], slot_of_agent[DDRL_MAXAG];
  int N, T, n_agents, W;           // W = ceil(N / 64) waves of envs
  const uint8_t* done_tn;
  int* cnt;                        // [T][W] episodes finished per (step, wave)
  long long* base;                 // [T][W] exclusive scan of cnt in (t, w) order
  long long* total;                // [1] sum of cnt
  double* ep_total;                // in-flight state of every env: [N] interleaved total,
  double* ep_agent;                //   [N][DDRL_MAXAG] per-agent totals,
  int* ep_len;                     //   [N] env steps
  double* table;                   // [cap][8]: {t, env, length, total, agent_0 .. agent_3}
  long long cap;
};
void launch_ep_count_scan(hipStream_t s, const EpArgs& a);   // cnt, base, total
void launch_ep_walk(hipStream_t s, const EpArgs& a);         // table rows + the in-flight state

// ---- group finish (finish_group.hip): GAE and the episode accounting of M contexts side by side ----
// The kernels of launch_gae, launch_ep_count_scan and launch_ep_walk with the member in blockIdx.z.
// What differs between members is one FinishMember in a device table; what is equal for all
// (sizes, record layouts, gamma / lambda, the agent maps) goes by value.
struct FinishMember {
  float* rec[DDRL_MAXP];
  const float* last_v[DDRL_MAXP];
  double* partials[DDRL_MAXP];     // GaeArgs::partials of each policy
  float* adv_norm[DDRL_MAXP];
  const uint8_t* done_tn;
  int* ep_cnt; long long* ep_base; long long* ep_word;
  double* ep_total; double* ep_agent; int* ep_len;
  double* ep_table; long long ep_cap;
};
struct FinishGroupArgs {
  const FinishMember* tab;         // device table of M members
  long long* totals;               // [M] episodes finished per member (the scan writes it)
  int M, P, T, N, W, n_agents;     // W = ceil(N / 64)
  int k[DDRL_MAXP], C[DDRL_MAXP];
  RecLayout lay[DDRL_MAXP];
  double gamma, lambda_;
  int policy_of_agent[DDRL_MAXAG], slot_of_agent[DDRL_MAXAG];
};
void launch_finish_group_gae(hipStream_t s, const FinishGroupArgs& fa);          // k_gae + finalize
void launch_finish_group_count_scan(hipStream_t s, const FinishGroupArgs& fa);   // cnt, base, totals
void launch_finish_group_walk(hipStream_t s, const FinishGroupArgs& fa);         // table rows + in-flight state

// ---- device env plane (devenv.hip; the dynamics are envdyn.h's) ----
// The env state is a struct of arrays: st[f][N], f = the first 38 entries of the packed layout
// (torso 10, q 8, qd 8, qfrc 8, foot 4) and the target velocity as field 38; steps and episode
// as integer arrays.
#define DDRL_DEVENV_FIELDS 39
struct DevEnvArgs {
  int N, D, time_limit, n_tv;
  unsigned long long seed;
  double* st;                // [DDRL_DEVENV_FIELDS][N]
  int* steps;                // [N]
  unsigned* episode;         // [N]
  const double* tv_list;     // [n_tv]
  const double* tv_env;      // [N] fixed target velocity of every env, or nullptr: drawn from tv_list
  float *obs, *fw, *cfrc, *kin;   // [N][D], [N], [N][14][6], [N][9]
  uint8_t* done;             // [N]
  // the ground (envdyn::Terrain): smoothness bounds, bump spacing and its inverse, generation;
  // ter_on: not flat (lo == hi == 1 is flat), which selects the terrain instance of the step kernel
  double ter_lo, ter_hi, ter_bump, ter_inv_bump;
  unsigned ter_gen;
  int ter_on;
};
enum { DEVENV_RESET_ALL = 0, DEVENV_RESET_EPISODES = 1, DEVENV_RESET_STATE = 2 };
// four lanes per env; the flat instance, or with a.ter_on the instance that evaluates the height
// field under every foot
void launch_devenv_step(hipStream_t s, const DevEnvArgs& a, const float* actions);
// out[n] = the ground height of env env_index[i] (its current episode's field) at (xy[2i], xy[2i+1])
void launch_devenv_terrain_height(hipStream_t s, const DevEnvArgs& a, const int* env_index, const double* xy, int n,
                                  double* out);
void launch_devenv_reset(hipStream_t s, const DevEnvArgs& a, int mode);
// packed[N][41] (DDRL_ENV_STATE_DOUBLES) <- state, or state <- packed when unpack
void launch_devenv_pack(hipStream_t s, const DevEnvArgs& a, double* packed, int unpack);

// ---- group rollout (rollout_group.hip): the device-plane fragments of M contexts side by side ----
// Member m is a context and its device env plane, separately allocated: everything that differs
// between members is one RolloutMember in a device table, indexed by blockIdx.z (wave-uniform);
// what is equal for all (routing, reward tables, record layout, sizes) goes by value.
struct RolloutMember {
  const float* theta[DDRL_MAXP];
  float* stage[DDRL_MAXP];
  float* rec[DDRL_MAXP];
  const float* cup[DDRL_MAXP];     // "cup" leg-coupling table [4][A] (nullptr: none)
  float* last_v[DDRL_MAXP];
  const float* eps;                // [T][n][n_agents][A] noise of the fragment
  float* actions;                  // [n][8]
  uint8_t* done_tn;                // [T][n]
  double *f_n, *f_M, *f_S, *f_normc, *f_dn, *f_dM, *f_dS, *f_part;   // env-side filter and its chunk scratch
  double* pf;                      // per-policy filter state [P][PF_STRIDE] (nullptr: disabled)
  double* zs;
  DevEnvArgs env;                  // the member's env plane: state, outputs, seed, time limit, velocities, terrain
};
struct RolloutGroupArgs {
  const RolloutMember* tab;        // device table of M members
  int M, n, T;                     // members, envs per member, fragment length
  RecLayout lay[DDRL_MAXP];
  int C[DDRL_MAXP];                // rows per step of each policy (n * k)
  int filter_update, filter_enabled, policy_filter;
  float clip;                      // effective clip of the env-side filter (0: none)
  int ter_on, tv_env;              // the step kernel's instance (equal for all members)
};
// one env step of every member: act(t) -> env step -> reward(t) -> filter push -> (policy filter) ->
// observe, the launch order of a plain device-plane step.  rw: the reward tables (rec / t unused / set here)
void launch_rollout_group_step(hipStream_t s, const RouteArgs& ra, const RewardArgs& rw, const RolloutGroupArgs& ga, int t);
// V(s_T) of every member into last_v
void launch_rollout_group_bootstrap(hipStream_t s, const RouteArgs& ra, const RolloutGroupArgs& ga);

// ---- device randomness (rng.hip; the generator and the layouts: philox.h) ----
// What differs between the members of a group fill is one entry of a device table, indexed by
// blockIdx.z; the solo kernels take the same struct by value.  The shapes are equal for all members.
struct NoiseMember {
  float* eps;                      // [n_steps][N][n_agents][A], 16-byte aligned
  unsigned long long seed, pos;    // the noise stream: its seed and the absolute step of eps[0]
};
// B: Philox blocks per env (n_agents * A / 4); one lane per block, one 16-byte store per lane
void launch_noise_fill(hipStream_t s, const NoiseMember& nm, int n_steps, int N, int B);
void launch_noise_fill_group(hipStream_t s, const NoiseMember* tab_dev, int M, int n_steps, int N, int B);
struct ScheduleMember {
  int32_t* shuffle[DDRL_MAXP];     // [R_p]
  int32_t* perm[DDRL_MAXP];        // [epochs][nb_p]
  unsigned long long seed, draw;   // the schedule stream: its seed and the index of this draw
};
struct ScheduleShape {
  int n_pol;                       // policies filled by the launch (the set bits of the mask) ...
  int pid[DDRL_MAXP];              // ... and their ids: blockIdx.y indexes this list
  int R[DDRL_MAXP], nb[DDRL_MAXP]; // by policy id
  int epochs;
};
// one lane per element of shuffle | perm[0] | perm[1] | ... of every filled policy
void launch_schedule_fill(hipStream_t s, const ScheduleMember& sm, const ScheduleShape& sh);
void launch_schedule_fill_group(hipStream_t s, const ScheduleMember* tab_dev, int M, const ScheduleShape& sh);

// ---- PPO update (fused persistent minibatch loop) ----
struct UpdateArgs {
  const float* rec; RecLayout lay;
  int d, A, R;                 // obs width, action dim, rows of this policy
  const int32_t* shuffle;      // [R]; null: the minibatch rows are rec[0 .. rows) (pre-gathered)
  const int32_t* perm;         // [E][nb]
  int nb, n_epochs, max_steps, step0;
  float* theta; float* m; float* v; float* beta_pow;   // beta_pow[2]
  float* stats;                // [steps][8]
  const float* adv_norm;       // [2]
  float* grad_out;             // optional: write raw (unclipped) grads and stop (DDP)
  float* gscr;                 // [n_params] gradient scratch (L2 resident)
  float kl_coeff;
  int cup;                     // "cup" model: the leg-coupling table follows the fcnet variables
};
struct UpdateHyper {
  float clip, vf_clip, vf_coeff, ent_coeff, lr, grad_clip, b1, b2, eps;
  int vf_mode;
  int P;
};
// ua: host array of h.P UpdateArgs (one persistent workgroup pair per entry), passed to the
//     kernel by value in its argument block (no device copy, nothing outlives the call)
// ksp: 1 = one workgroup per branch, 2 = row split over two (gx: gx_bytes(P) of exchange granules)
// d / stride: the widest obs width / record stride of the launched policies
// own_kq: -1 = both row halves in this launch; 0 / 1 = peer mode (that half only; gx shared with
// the peer context, whose launch runs the other half; launch_update_ffn_peer)
// lx_base: peer mode's global step count before this launch (0 otherwise)
void launch_update_ffn(hipStream_t s, const UpdateArgs* ua, const UpdateHyper& h, int nrows, float inv_n, int A, int d,
                       int stride, int cup, unsigned long long* xchg, unsigned long long* gx, int ksp, int* err,
                       unsigned* epoch_ctr, int* xcc, int own_kq = -1, unsigned lx_base = 0);
// the same with the relaxed system-scope atomic exchange (ppo_ffn_atomic.hip): any placement
void launch_update_ffn_atomic(hipStream_t s, const UpdateArgs* ua, const UpdateHyper& h, int nrows, float inv_n, int A,
                              int d, int stride, int cup, unsigned long long* xchg, unsigned long long* gx, int ksp,
                              int* err, unsigned* epoch_ctr, int* xcc, int own_kq = -1, unsigned lx_base = 0);
// the launches of launch_update_ffn other than the fused row split: KSP = 1 and gradient export (ppo_ffn_k1.hip)
void launch_update_ffn_k1(hipStream_t s, const UpdateArgs* ua, const UpdateHyper& h, int nrows, float inv_n, int A,
                          int d, int stride, int cup, unsigned long long* xchg, unsigned long long* gx, int ksp,
                          int* err, unsigned* epoch_ctr, int* xcc, int own_kq = -1, unsigned lx_base = 0);
// peer mode (ppo_ffn_peer.hip): the LSB-tagged quads at system scope, outboxes shared with the
// peer context's launch (fine-grained memory a peer GPU reads)
void launch_update_ffn_peer(hipStream_t s, const UpdateArgs* ua, const UpdateHyper& h, int nrows, float inv_n, int A,
                            int d, int stride, int cup, unsigned long long* xchg, unsigned long long* gx, int ksp,
                            int* err, unsigned* epoch_ctr, int* xcc, int own_kq = -1, unsigned lx_base = 0);
// sgd_minibatch_size = 256 (ppo_ffn_mb256.hip / ppo_ffn_mb256_atomic.hip, the header built with
// DDRL_MB = 256): fused row-split launches of whole minibatches only -- ksp = 2, nrows = 256, no
// gradient export, own_kq = -1; anything else sets the error word and launches nothing
void launch_update_ffn_mb256(hipStream_t s, const UpdateArgs* ua, const UpdateHyper& h, int nrows, float inv_n, int A,
                             int d, int stride, int cup, unsigned long long* xchg, unsigned long long* gx, int ksp,
                             int* err, unsigned* epoch_ctr, int* xcc, int own_kq = -1, unsigned lx_base = 0);
void launch_update_ffn_mb256_atomic(hipStream_t s, const UpdateArgs* ua, const UpdateHyper& h, int nrows, float inv_n,
                                    int A, int d, int stride, int cup, unsigned long long* xchg,
                                    unsigned long long* gx, int ksp, int* err, unsigned* epoch_ctr, int* xcc,
                                    int own_kq = -1, unsigned lx_base = 0);
// epoch_ctr: per-context launch counter (granule tags)
size_t gx_bytes(int P);
// The group update (ppo_ffn_group.hip): n_chains chains (one policy of one member context each) in
// one launch of the fused row-split kernel, 128-row minibatches, default protocol, every chain from
// schedule step 0.  table_dev: device array of n_chains UpdateArgs; xchg: 8 granules per chain,
// rounded up to whole group rows of 8 chains; gx: gx_bytes(n_chains); xcc: update_group_grid(n_chains)
// ints; epoch_ctr: the group's launch counter.  Clears the outboxes on the stream first.  Returns
// -1 (nothing launched) in a library built without the group kernel.
int update_group_grid(int n_chains);   // blocks of a launch: 32 (rows - 1) + 24 + chains in the last row
int launch_update_ffn_group(hipStream_t s, const UpdateArgs* table_dev, int n_chains, const UpdateHyper& h, int A, int d,
                            int stride, int cup, unsigned long long* xchg, unsigned long long* gx, int* err,
                            unsigned* epoch_ctr, int* xcc);
// clip_by_global_norm + tf1 Adam on a flat (all-reduced) gradient vector
// gscale multiplies the gradient before the clip (1 / ranks in the "local" data-parallel mode)
// err: the context's error word -- a set word (a failed gradient launch) skips the update
void launch_apply_adam(hipStream_t s, const float* grad, int n, float* theta, float* m, float* v,
                       float* beta_pow, const UpdateHyper& h, float gscale, int xcd, const int* err);
// Bounds-checked diagnostic build (-DDDRL_BOUNDS): violation counters of the update kernel's
// staging / record / schedule / LDS indices (see ppo_ffn.hip); ddrl_diag_bounds reads them.
#define DDRL_NBOUNDS 6

// ---- ModelV2.forward / value_function on arbitrary rows ----
struct ForwardArgs {
  const float* theta; const float* x; const int32_t* node; int n, d, A;
  const float* cup;             // ffn: leg-coupling table [4][A] ("cup" model) or nullptr
  float* logits; float* values;
};
void launch_forward_ffn(hipStream_t s, const ForwardArgs& fa);
int ffn_param_count(int d, int A);       // fcnet variables of one policy (ffn.h ffn_offsets)
void launch_forward_gnn(hipStream_t s, const ForwardArgs& fa, int layer);

// ---- GraphNet (gnn.hip): per-tile kernels, one minibatch step = grad / reduce / Adam ----
struct GnnArgs {
  const float* theta;
  int n_graphs;                 // envs (act), rows (forward) or minibatch rows (grad)
  const float* x;               // act: stage [N][4][23]; forward: [n][4][23]
  const int32_t* node;          // forward: node of every row
  // act
  float* rec; RecLayout lay; int t; const float* eps; float* actions; int n_agents;
  int act_index[4][8]; int bootstrap; float* last_v;
  // forward
  float* logits; float* values;
  // grad
  UpdateArgs u; UpdateHyper h; int step; float inv_n;
  float* part; int part_stride;  // [tiles][n_params] partial gradients
  float* statp;                  // [2 nets][32 tiles][8]
  float* normp;                  // [reduce blocks] squared-norm partials
  float* bp_cur;                 // [2] beta powers of the current step
  float* grad;                   // reduced gradient (scratch or the DDP output)
  int act_e0, act_nfull;          // act: first env of the range, envs of the shard (record rows)
  // staged minibatch (fused update only): the records of this step, contiguous [128][stride]
  // (a slot of the pre-gathered chunk); null: gather through shuffle / perm
  const float* stage;
  // one-launch step (gnn.hip gnn_tail): arrival flags [256], norm^2 granules [256], this launch's
  // tag; the XCD-grouped 1-D grid (xgrid); the parameters of each (net, share) combination
  // (plist[poff[k] .. poff[k + 1]), k = 4 net + share) and the first reducer index of each (rbase)
  unsigned* flags; unsigned long long* gran; unsigned tag; int tail; int nred; int n_params; int ntiles; int* err;
  // xgrid: 1 = the XCD-grouped grid, 2 = test hook remapping each combination across every XCD;
  // xcc: [8 combinations][32 tiles] XCC id of the workgroup that ran each tile (placement record)
  int xgrid; int only_share; const int* plist; int poff[9]; int rbase[9]; int* xcc;
};
struct GnnScratch {
  float* part; int part_stride; float* statp; float* normp; float* bp_cur; float* grad;
  float* chunk;       // [chunk_steps][128][stride] records of a run of minibatch steps
  int chunk_steps;    // min(GNN_CHUNK_STEPS, the schedule's steps); chunk allocated on first use
  unsigned* flags;              // [256] arrival flags of the one-launch step (device)
  unsigned long long* gran;     // [256] tagged norm^2 partials {value, tag} of its reduction blocks
  unsigned seq;                 // tag of the last one-launch step (host; never 0)
  int* plist;                   // [n_params] parameters by (net, share) owner (device)
  int poff[9], rbase[9];        // list offsets / first reducer of each combination
  int lists;                    // 0: not built yet, 1: built, -1: unusable (three launches)
  int tail;           // 1: reduction + clip + Adam in the gradient launch (DDRL_GNN_TAIL, default 1)
  int* err;           // the context's error word
  int* xcc;           // [256] XCC id per (combination, tile) of the last one-launch step (device)
  int xcc_pending;    // a one-launch step ran since the host last checked its placement
  int misplace;       // test hook (DDRL_TEST_GNN_MISPLACE): every combination straddles the XCDs
};
#define GNN_CHUNK_STEPS 1024
int gnn_param_total(int A, int layer);   // layer: DDRL_GNN_*
// stage: the step's pre-gathered records (fused update) or null (data-parallel gradient of
// explicit rows)
void launch_step_gnn(hipStream_t s, const UpdateArgs& u, const UpdateHyper& h, int step, int nrows, float inv_n,
                     GnnScratch& sc, const float* stage, int layer);
// the records of minibatch steps [step0, step0 + n_steps) of the schedule -> dst
// ([n_steps][128][stride], n_steps <= GNN_CHUNK_STEPS): one bandwidth-bound gather per chunk
void launch_gnn_gather(hipStream_t s, const UpdateArgs& u, int step0, int n_steps, float* dst);
// data-parallel steps: step k's m minibatch rows gathered into dst[k][m][stride] (ppo_ffn.hip)
void launch_rows_gather(hipStream_t s, const float* rec, int stride, const int32_t* shuffle, const int32_t* perm,
                        int m, int step0, int n_steps, float* dst);
