// C-ABI of libddrl_hip.so (declared in include/ddrl_hip.h).
// Owns every device buffer of a training shard; all work is enqueued on one HIP stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/ddrl_hip.h"
#include "hostenv.h"
#include "kernels.h"

namespace {
thread_local std::string g_err;

int fail(const std::string& msg) {
  g_err = msg;
  return -1;
}

#define HIPCHK(x)                                                                   \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess)                                                           \
      return fail(std::string(#x) + ": " + hipGetErrorString(e_));                  \
  } while (0)

#define NCCLCHK(x)                                                                  \
  do {                                                                              \
    ncclResult_t r_ = (x);                                                          \
    if (r_ != ncclSuccess) return fail(std::string(#x) + ": " + ncclGetErrorString(r_)); \
  } while (0)

#define CHK_CTX(c) \
  if (!(c)) return fail("null context")

int gnn_param_count(int A, int layer) { return gnn_param_total(A, layer); }

struct Policy {
  int k = 0, d = 0, C = 0, n_params = 0, R = 0, nb = 0;
  int agents[DDRL_MAXAG] = {0};
  RecLayout lay{};
  float *theta = nullptr, *m = nullptr, *v = nullptr, *beta_pow = nullptr;
  float *rec = nullptr, *stage = nullptr, *last_v = nullptr, *adv_norm = nullptr;
  float *stats = nullptr, *grad = nullptr;
  double* partials = nullptr;
  int last_steps = 0;
  size_t stats_steps = 0;   // rows of `stats` (num_sgd_iter * nb; peer mode may grow it)
};
}  // namespace

// the member tables of the group fills a context led (device randomness, at the end of this file)
struct RngTables;
static void rng_tables_free(RngTables* t);

struct ddrl_ctx {
  ddrl_cfg cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  Policy pol[DDRL_MAXP];
  RouteArgs route{};
  double *f_n = nullptr, *f_M = nullptr, *f_S = nullptr, *f_normc = nullptr;
  double *f_dn = nullptr, *f_dM = nullptr, *f_dS = nullptr;   // pushes since the last sync
  double* f_part = nullptr;                                     // filter push chunk scratch
  double* pf = nullptr;   // per-policy RLlib MeanStdFilter state [P][PF_STRIDE]
  double* zs = nullptr;   // fp64 column sums of the env-normalized observation [2][D]
  uint8_t* done_tn = nullptr;
  float** stage_tab = nullptr;    // device array of per-policy stage pointers
  int32_t* zero_perm = nullptr;
  unsigned long long* xchg = nullptr;  // norm^2 exchange granules of the update kernel
  unsigned long long* gx = nullptr;    // partial-gradient granules of the row-split update
  unsigned upd_epoch = 0;              // update launches so far (granule tag epochs)
  int update_split = 2;                // workgroups per branch of the fused update (1 or 2)
  int* err = nullptr;                  // device error word (exchange timeout)
  // Placement / rollback (fcnet update): the XCC of every block of the last update launch,
  // the exchange protocol (0: plain stores into the XCD's L2, 1: relaxed agent-scope atomics,
  // chosen by DDRL_XCHG=atomic or after a placement failure), and per policy a snapshot of
  // theta | m | v | beta powers taken before each update, restored when the launch fails.
  int* xcc = nullptr;
  int xchg_atomic = 0;
  int xcc_pending = 0;                 // blocks of an update launch not yet checked (grid size)
  int xcc_ksp = 2;
  int xcc_mask = 0;
  int fail_step = -1;                  // test hook: DDRL_TEST_FAIL_STEP
  float* snap[DDRL_MAXP] = {nullptr};
  int snap_mask = 0;
  float kl_last[DDRL_MAXP] = {0};
  GnnScratch gnn{};               // GraphNet step scratch (per-tile partial gradients, ...)
  // host-variant staging
  float *h_obs = nullptr, *h_eps = nullptr, *h_act = nullptr;
  ncclComm_t comm = nullptr;           // data-parallel learner (ddrl_comm_init)
  float* ddp_chunk = nullptr;          // ddrl_ppo_update_ddp: pre-gathered records of a run of steps
  size_t ddp_chunk_n = 0;
  int32_t* ddp_slots = nullptr;        // ... and the minibatch slot of every step (device copy)
  size_t ddp_slots_n = 0;
  std::vector<int32_t> ddp_slots_host; // source of that copy, alive until the call's final sync
  float *h_fw = nullptr, *h_cfrc = nullptr;
  uint8_t* h_done = nullptr;
  // ddrl_rollout_fragment as one HIP graph (T x (act, reward, filter push, observe) +
  // bootstrap), captured on first use and re-used while the call's buffers are the same
  // (every other kernel argument is fixed at context creation); DDRL_ROLLOUT_GRAPH=0: launches
  int rollout_graph = 1;
  hipGraphExec_t rg_exec = nullptr;
  hipStream_t cap_stream = nullptr;    // capture only (the caller's stream may be the null stream)
  const void* rg_key[6] = {nullptr};
  // peer mode (ddrl_ppo_update_peer): the outboxes shared with the peer context, this context's
  // row half, the launch tags both contexts step in lockstep, the IPC mapping to close, and the
  // per-rank virtual shuffle ([nb][128] row indices, this rank's rows in half peer_rank)
  void* peer_gx = nullptr;
  int peer_rank = -1;
  unsigned peer_epoch = 0;
  unsigned peer_steps = 0;   // steps the attached pair has run (the quads' tag bit and outbox parity)
  int peer_inflight = 0;     // a peer launch is enqueued and not yet checked (check_err)
  void* peer_ipc = nullptr;
  int32_t* peer_vsh = nullptr;
  size_t peer_vsh_n = 0;
  // evaluation (ddrl_eval_*): per-env fp64 accumulators, episode counts, the result table
  // [N][E][6], the two progress counters and the device copy of the env plane's kin buffer;
  // ev_normc_ok: the filter constants are known current (no push since they were written)
  int ev_on = 0;
  ddrl_eval_cfg ev_cfg{};
  double *ev_acc = nullptr, *ev_table = nullptr;
  int32_t* ev_count = nullptr;
  unsigned long long* ev_ctr = nullptr;
  float* ev_kin = nullptr;
  int ev_table_E = 0;
  int ev_normc_ok = 0;
  // evaluation members (ddrl_eval_members_*): mem_on = M while the mode is on, member m owns the
  // envs [m n, (m + 1) n).  Per member: the flat parameters of every policy (mem_theta[p], stride
  // mem_tstride[p] floats), the env-side filter block (FM_* layout), the per-policy filter state
  // [P][PF_STRIDE] and the chunk scratch of the filter push.  mem_cap: the M the buffers hold;
  // mem_normc_ok: every member's filter constants are current
  int mem_on = 0, mem_cap = 0, mem_normc_ok = 0;
  float* mem_theta[DDRL_MAXP] = {nullptr};
  size_t mem_tstride[DDRL_MAXP] = {0};
  double *mem_filt = nullptr, *mem_pf = nullptr, *mem_part = nullptr;
  std::vector<char> mem_loaded;
  // input sensitivity (ddrl_eval_sens_*): the steps [P][DDRL_MAXD], per policy the per-base-row
  // accumulators [C][2][d][A] and step counts [C], the reduced result; sens_act_ok: a
  // ddrl_eval_act has run since the filter constants may last have changed
  int sens_on = 0, sens_act_ok = 0;
  double* sens_step = nullptr;
  double* sens_acc[DDRL_MAXP] = {nullptr};
  long long* sens_cnt[DDRL_MAXP] = {nullptr};
  double* sens_red = nullptr;      // [2 * DDRL_MAXD * 8] + one int64
  // episode accounting (ddrl_episodes_*), allocated by the first call: the in-flight state of
  // every env (interleaved total, per-agent totals, length), the per-(step, wave) counts and
  // their scan, the table of the last collect (ep_cap rows of 8 doubles, ep_rows written);
  // ep_collected: the fragment the context holds has been walked (rewards / records re-arm it)
  double *ep_total = nullptr, *ep_agent = nullptr, *ep_table = nullptr;
  int *ep_len = nullptr, *ep_cnt = nullptr;
  long long *ep_base = nullptr, *ep_word = nullptr;
  long long ep_cap = 0, ep_rows = -1;
  int ep_collected = 0;
  // device env planes bound to this context (ddrl_devenv_*), and ddrl_rollout_devenv's graph:
  // keyed by the env's id, its settings generation and the noise buffer
  std::vector<ddrl_devenv*> devenvs;
  hipGraphExec_t rgd_exec = nullptr;
  uint64_t rgd_env = 0;
  unsigned rgd_gen = 0;
  const void* rgd_eps = nullptr;
  // device randomness (ddrl_rng_*): the noise and the schedule stream (DDRL_RNG_*), each a seed and
  // a position, all of the generator's state; unseeded streams refuse every draw
  struct RngStream { uint64_t seed = 0, pos = 0; int seeded = 0; } rng[2];
  RngTables* rng_tabs = nullptr;   // allocated by the first group fill with this context as member 0
  std::vector<void*> allocs;
};

// A device env plane (devenv.hip): the kernel arguments (state and output buffers in device
// memory), the host copy of the target-velocity list and the scratch of state_get / state_set.
struct ddrl_devenv {
  ddrl_ctx* ctx = nullptr;       // null once the context is gone
  uint64_t id = 0;               // unique per process (a graph key must not be an address that is reused)
  unsigned gen = 0;              // bumped by every setting a captured launch has baked in
  DevEnvArgs a{};
  std::vector<double> tv_list;
  double* tv_dev = nullptr;
  size_t tv_cap = 0;
  double* tv_env_dev = nullptr;   // [N] per-env velocities (set_env_target_velocities), allocated on first use
  double* packed = nullptr;
  std::vector<void*> allocs;
};

template <class T>
static bool env_alloc(ddrl_devenv* e, T** p, size_t count) {
  void* ptr = nullptr;
  const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  if (hipMalloc(&ptr, bytes) != hipSuccess) return false;
  e->allocs.push_back(ptr);
  *p = static_cast<T*>(ptr);
  return hipMemset(ptr, 0, bytes) == hipSuccess;
}

template <class T>
static int dalloc(ddrl_ctx* c, T** p, size_t count) {
  void* ptr = nullptr;
  const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  hipError_t e = hipMalloc(&ptr, bytes);
  if (e != hipSuccess) return fail(std::string("hipMalloc failed: ") + hipGetErrorString(e));
  e = hipMemset(ptr, 0, bytes);
  if (e != hipSuccess) return fail(std::string("hipMemset failed: ") + hipGetErrorString(e));
  c->allocs.push_back(ptr);
  *p = static_cast<T*>(ptr);
  return 0;
}

// a buffer that is replaced by a larger one (the data-parallel loop's chunk and slots): the
// callers run after a stream synchronize, so nothing in flight still reads it
template <class T>
static void dfree(ddrl_ctx* c, T** p) {
  if (!*p) return;
  auto it = std::find(c->allocs.begin(), c->allocs.end(), static_cast<void*>(*p));
  if (it != c->allocs.end()) c->allocs.erase(it);
  (void)hipFree(*p);
  *p = nullptr;
}

static RecLayout make_layout(const ddrl_cfg& cfg, int d) {
  RecLayout L;
  const int A = cfg.act_dim;
  L.obs = 0;
  const int obs_len = cfg.model_kind == DDRL_MODEL_GNN ? 4 * 23 + 1 : d;
  L.act = obs_len;
  L.logit = L.act + A;
  L.logp = L.logit + 2 * A;
  L.vf = L.logp + 1;
  L.adv = L.vf + 1;
  L.vt = L.adv + 1;
  L.rew = L.vt + 1;
  L.cid = cfg.leg_coupling ? L.rew + 1 : -1;   // "cup": the row's leg index (coupling row)
  L.stride = ((cfg.leg_coupling ? L.cid : L.rew) + 1 + 3) & ~3;
  return L;
}

static int validate(const ddrl_cfg& c) {
  if (c.n_envs <= 0 || c.frag_len <= 0) return fail("n_envs and frag_len must be positive");
  if (c.n_policies < 1 || c.n_policies > DDRL_MAXP) return fail("n_policies must be in [1, 4]");
  if (c.n_agents < 1 || c.n_agents > DDRL_MAXAG) return fail("n_agents must be in [1, 4]");
  if (c.act_dim != 2 && c.act_dim != 4 && c.act_dim != 8) return fail("act_dim must be 2, 4 or 8");
  if (c.obs_full_dim < 1 || c.obs_full_dim > DDRL_MAXFULL) return fail("obs_full_dim out of range");
  // the fused update kernels are built per minibatch size: 128 rows for every model, 256 for the
  // fcnet models (ppo_ffn_mb256.hip)
  if (c.model_kind == DDRL_MODEL_GNN && c.sgd_minibatch_size != 128)
    return fail("sgd_minibatch_size must be 128 for the GraphNet model (its update kernels are built for 128 rows)");
  if (c.sgd_minibatch_size != 128 && c.sgd_minibatch_size != 256)
    return fail("sgd_minibatch_size must be 128 or 256 (the fused update kernels are built for these two)");
  if (c.num_sgd_iter < 1) return fail("num_sgd_iter must be >= 1");
  // hyperparameters that can only produce NaN parameters: a NaN itself, and grad_clip <= 0 (the clip
  // scale is grad_clip * min(1 / norm, 1 / grad_clip)).  lr 0 and grad_clip 1e30 (no clipping) are legal.
  const struct { const char* name; float v; } hyper[] = {
      {"gamma", c.gamma}, {"lambda_", c.lambda_}, {"clip_param", c.clip_param}, {"vf_clip_param", c.vf_clip_param},
      {"vf_loss_coeff", c.vf_loss_coeff}, {"entropy_coeff", c.entropy_coeff}, {"lr", c.lr}, {"grad_clip", c.grad_clip},
      {"adam_beta1", c.adam_beta1}, {"adam_beta2", c.adam_beta2}, {"adam_eps", c.adam_eps}};
  for (const auto& h : hyper)
    if (std::isnan(h.v)) return fail(std::string(h.name) + " is NaN");
  if (!(c.grad_clip > 0.f)) return fail("grad_clip must be > 0 (pass 1e30 for no clipping)");
  for (int j = 0; j < c.n_agents; ++j)
    if (c.agent_policy[j] < 0 || c.agent_policy[j] >= c.n_policies) return fail("bad agent_policy");
  for (int p = 0; p < c.n_policies; ++p) {
    const int d = c.obs_dim[p];
    if (d < 1 || d > DDRL_MAX_OBS) return fail("obs_dim out of range");
    if (c.model_kind == DDRL_MODEL_FFN && d > 48) return fail("ffn obs_dim must be <= 48");
  }
  if (c.model_kind == DDRL_MODEL_GNN && (c.n_policies != 1 || c.n_agents != 4 || c.obs_dim[0] != 19))
    return fail("gnn requires one shared leg policy, 4 agents and 19 features per node");
  if (c.model_kind == DDRL_MODEL_GNN && c.act_dim != 2) return fail("gnn kernels are built for act_dim 2");
  if (c.gnn_layer < DDRL_GNN_MPNN || c.gnn_layer > DDRL_GNN_GAT1) return fail("gnn_layer must be one of DDRL_GNN_*");
  if (c.leg_coupling && (c.model_kind != DDRL_MODEL_FFN || c.act_dim != 2 || c.n_policies != 1 || c.n_agents != 4 ||
                          c.obs_dim[0] > 20))
    return fail("leg_coupling (\"cup\") requires the fcnet model, one shared leg policy, 4 agents, act_dim 2 and obs_dim <= 20");
  if (c.policy_filter && c.model_kind != DDRL_MODEL_FFN)
    return fail("the per-policy MeanStdFilter is built for fcnet policies (flat observations)");
  for (int j = 0; j < c.n_agents; ++j) {
    const int d = c.obs_dim[c.agent_policy[j]];
    for (int f = 0; f < d; ++f)
      if (c.obs_index[j][f] < -2 || c.obs_index[j][f] >= c.obs_full_dim ||
          (c.model_kind == DDRL_MODEL_GNN && c.obs_index[j][f] < 0))
        return fail("bad obs_index");
      else if (c.policy_filter && c.obs_index[j][f] < 0)
        return fail("constant input columns (LegID) with the per-policy MeanStdFilter are not supported");
    if (c.n_contact[j] < 0 || c.n_contact[j] > 14) return fail("bad n_contact");
    for (int b = 0; b < c.n_contact[j]; ++b)
      if (c.contact_index[j][b] < 0 || c.contact_index[j][b] >= 14) return fail("bad contact_index");
    for (int a = 0; a < c.act_dim; ++a)
      if (c.act_index[j][a] < 0 || c.act_index[j][a] >= 8) return fail("bad act_index");
  }
  return 0;
}

extern "C" {

int ddrl_abi_version(void) { return DDRL_ABI_VERSION; }
const char* ddrl_last_error(void) { return g_err.c_str(); }

int ddrl_ctx_create(const ddrl_cfg* cfg, int device, ddrl_ctx** out) {
  if (!cfg || !out) return fail("null argument");
  if (validate(*cfg)) return -1;
  // fused update geometry: DDRL_UPDATE_SPLIT=1 keeps one workgroup per branch (timing / A-B)
  int update_split = 2;
  if (const char* e = std::getenv("DDRL_UPDATE_SPLIT")) update_split = std::atoi(e) == 1 ? 1 : 2;
  if (update_split != 2 && cfg->sgd_minibatch_size != 128)
    return fail("sgd_minibatch_size 256 needs the row split: DDRL_UPDATE_SPLIT=1 would put 256-row images in one "
                "workgroup, which its LDS cannot hold");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail("device index out of range");
  HIPCHK(hipSetDevice(device));
  ddrl_ctx* c = new ddrl_ctx();
  c->update_split = update_split;
  c->cfg = *cfg;
  c->device = device;
  const ddrl_cfg& g = c->cfg;
  const int N = g.n_envs, T = g.frag_len;
  RouteArgs& ra = c->route;
  ra.P = g.n_policies; ra.N = N; ra.A = g.act_dim; ra.full_dim = g.obs_full_dim;
  ra.n_agents = g.n_agents; ra.model = g.model_kind;
  for (int j = 0; j < 4; ++j) ra.leg_angle[j] = g.leg_angle_deg[j];
  int rc = 0;
  for (int p = 0; p < g.n_policies && !rc; ++p) {
    Policy& P = c->pol[p];
    P.d = g.obs_dim[p];
    for (int j = 0; j < g.n_agents; ++j)
      if (g.agent_policy[j] == p) P.agents[P.k++] = j;
    if (P.k == 0) { rc = fail("policy without agents"); break; }
    P.C = N * P.k;
    P.R = T * P.C;
    P.nb = std::max(1, P.R / g.sgd_minibatch_size);
    P.lay = make_layout(g, P.d);
    P.n_params = g.model_kind == DDRL_MODEL_FFN ? ffn_param_count(P.d, g.act_dim) : gnn_param_count(g.act_dim, g.gnn_layer);
    if (g.leg_coupling) P.n_params += 4 * g.act_dim;   // leg_coupling [4][A] after the fcnet variables
    PolicyRoute& pr = ra.pol[p];
    pr.k = P.k; pr.d = P.d;
    for (int s = 0; s < P.k; ++s) {
      pr.agent[s] = P.agents[s];
      for (int f = 0; f < DDRL_MAXD; ++f) pr.obs_index[s][f] = g.obs_index[P.agents[s]][f];
      pr.act_neg[s] = 0;
      for (int a = 0; a < 8; ++a) {
        pr.act_index[s][a] = g.act_index[P.agents[s]][a];
        if (g.act_negate[P.agents[s]][a]) pr.act_neg[s] |= 1 << a;
      }
    }
    const size_t stage_n = g.model_kind == DDRL_MODEL_GNN ? (size_t)N * 4 * 23 : (size_t)P.C * P.d;
    rc = rc || dalloc(c, &P.theta, P.n_params) || dalloc(c, &P.m, P.n_params) ||
         dalloc(c, &P.v, P.n_params) || dalloc(c, &P.beta_pow, 4) || dalloc(c, &P.grad, P.n_params) ||
         dalloc(c, &P.rec, (size_t)P.R * P.lay.stride) || dalloc(c, &P.stage, stage_n) ||
         dalloc(c, &P.last_v, P.C) || dalloc(c, &P.adv_norm, 2) ||
         dalloc(c, &P.partials, (size_t)gae_partials_len(P.C)) ||
         dalloc(c, &P.stats, (size_t)g.num_sgd_iter * P.nb * 8);
    P.stats_steps = (size_t)g.num_sgd_iter * P.nb;
    if (!rc) {
      // beta1^t, beta2^t, then the arrival counter of the multi-workgroup apply kernel (0)
      float bp[4] = {g.adam_beta1, g.adam_beta2, 0.f, 0.f};
      if (hipMemcpy(P.beta_pow, bp, sizeof(bp), hipMemcpyHostToDevice) != hipSuccess) rc = fail("init beta_pow");
      float an[2] = {0.f, 1.f};
      if (hipMemcpy(P.adv_norm, an, sizeof(an), hipMemcpyHostToDevice) != hipSuccess) rc = fail("init adv_norm");
    }
  }
  rc = rc || dalloc(c, &c->f_n, 1) || dalloc(c, &c->f_M, DDRL_MAXFULL) || dalloc(c, &c->f_S, DDRL_MAXFULL) ||
       dalloc(c, &c->f_normc, 2 * DDRL_MAXFULL) || dalloc(c, &c->f_dn, 1) ||
       dalloc(c, &c->f_dM, DDRL_MAXFULL) || dalloc(c, &c->f_dS, DDRL_MAXFULL) ||
       dalloc(c, &c->f_part, filter_part_doubles(N, DDRL_MAXFULL)) ||
       dalloc(c, &c->pf, (size_t)DDRL_MAXP * PF_STRIDE) || dalloc(c, &c->zs, 2 * DDRL_MAXFULL) || dalloc(c, &c->done_tn, (size_t)T * N) ||
       dalloc(c, &c->stage_tab, DDRL_MAXP) || dalloc(c, &c->zero_perm, 4) ||
       dalloc(c, &c->xchg, 8 * DDRL_MAXP) ||
       dalloc(c, &c->gx, gx_bytes(DDRL_MAXP) / sizeof(unsigned long long)) || dalloc(c, &c->err, 1) ||
       dalloc(c, &c->xcc, 32) ||
       dalloc(c, &c->h_obs, (size_t)N * g.obs_full_dim) ||
       dalloc(c, &c->h_eps, (size_t)N * g.n_agents * g.act_dim) || dalloc(c, &c->h_act, (size_t)N * 8) ||
       dalloc(c, &c->h_fw, N) || dalloc(c, &c->h_cfrc, (size_t)N * 14 * 6) || dalloc(c, &c->h_done, N);
  for (int p = 0; p < g.n_policies && !rc; ++p)
    rc = dalloc(c, &c->snap[p], 3 * (size_t)c->pol[p].n_params + 4);
  if (const char* e = std::getenv("DDRL_XCHG")) c->xchg_atomic = std::string(e) == "atomic" ? 1 : 0;
  if (const char* e = std::getenv("DDRL_TEST_FAIL_STEP")) c->fail_step = std::atoi(e);
  if (const char* e = std::getenv("DDRL_ROLLOUT_GRAPH")) c->rollout_graph = std::atoi(e) != 0;
  if (!rc && g.model_kind == DDRL_MODEL_GNN) {
    const int np = c->pol[0].n_params;
    c->gnn.part_stride = (np + 3) & ~3;   // 16-byte aligned tile rows (float4 partial stores)
    c->gnn.grad = c->pol[0].grad;
    rc = dalloc(c, &c->gnn.part, (size_t)(DDRL_MB / 4) * c->gnn.part_stride) || dalloc(c, &c->gnn.statp, 2 * (DDRL_MB / 4) * 8) ||
         dalloc(c, &c->gnn.normp, (np + 255) / 256) || dalloc(c, &c->gnn.bp_cur, 2) || dalloc(c, &c->gnn.flags, 256) ||
         dalloc(c, &c->gnn.gran, 256) || dalloc(c, &c->gnn.plist, np) || dalloc(c, &c->gnn.xcc, 256);
    c->gnn.seq = 0;
    c->gnn.lists = 0;
    c->gnn.err = c->err;
    c->gnn.tail = 1;
    c->gnn.xcc_pending = 0;
    c->gnn.misplace = 0;
    if (const char* e = std::getenv("DDRL_GNN_TAIL")) c->gnn.tail = std::atoi(e) != 0;
    if (const char* e = std::getenv("DDRL_TEST_GNN_MISPLACE")) c->gnn.misplace = std::atoi(e) != 0;
    // the record chunk of the fused update is allocated by the first ddrl_ppo_update (forward-only
    // and data-parallel contexts never need it), sized to the schedule when that is shorter
    c->gnn.chunk = nullptr;
    c->gnn.chunk_steps = std::min(GNN_CHUNK_STEPS, g.num_sgd_iter * c->pol[0].nb);
  }
  if (!rc) {
    float* tab[DDRL_MAXP] = {nullptr};
    for (int p = 0; p < g.n_policies; ++p) tab[p] = c->pol[p].stage;
    if (hipMemcpy(c->stage_tab, tab, sizeof(tab), hipMemcpyHostToDevice) != hipSuccess) rc = fail("stage table");
  }
  if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail("device sync after init");
  if (rc) {
    ddrl_ctx_destroy(c);
    return -1;
  }
  *out = c;
  return 0;
}

int ddrl_ctx_destroy(ddrl_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  if (c->comm) (void)ncclCommDestroy(c->comm);
  if (c->peer_ipc) (void)hipIpcCloseMemHandle(c->peer_ipc);
  if (c->rg_exec) (void)hipGraphExecDestroy(c->rg_exec);
  if (c->rgd_exec) (void)hipGraphExecDestroy(c->rgd_exec);
  for (ddrl_devenv* e : c->devenvs) e->ctx = nullptr;   // orphaned: only destroy is left to them
  if (c->cap_stream) (void)hipStreamDestroy(c->cap_stream);
  if (c->rng_tabs) rng_tables_free(c->rng_tabs);
  for (void* p : c->allocs) (void)hipFree(p);
  delete c;
  return 0;
}

int ddrl_set_stream(ddrl_ctx* c, void* s) {
  CHK_CTX(c);
  c->stream = static_cast<hipStream_t>(s);
  return 0;
}

// Snapshot of the policies an fcnet update launch is about to change (stream-ordered D2D copies:
// theta | m | v | beta powers), restored by check_err when the launch fails.
static int snapshot(ddrl_ctx* c, int mask) {
  for (int p = 0; p < c->cfg.n_policies; ++p) {
    if (!(mask & (1 << p)) || !c->snap[p]) continue;
    Policy& P = c->pol[p];
    const size_t n = (size_t)P.n_params;
    HIPCHK(hipMemcpyAsync(c->snap[p], P.theta, n * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->snap[p] + n, P.m, n * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->snap[p] + 2 * n, P.v, n * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->snap[p] + 3 * n, P.beta_pow, 4 * 4, hipMemcpyDeviceToDevice, c->stream));
  }
  c->snap_mask = mask;
  return 0;
}

static int restore_snapshot(ddrl_ctx* c) {
  for (int p = 0; p < c->cfg.n_policies; ++p) {
    if (!(c->snap_mask & (1 << p)) || !c->snap[p]) continue;
    Policy& P = c->pol[p];
    const size_t n = (size_t)P.n_params;
    HIPCHK(hipMemcpyAsync(P.theta, c->snap[p], n * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.m, c->snap[p] + n, n * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.v, c->snap[p] + 2 * n, n * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.beta_pow, c->snap[p] + 3 * n, 4 * 4, hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// The default exchange protocol needs the workgroups of one policy (blocks p, p + 8, ... of the
// launch) on one XCD.  Returns 1 if the last launch's recorded XCC ids (HW_REG_XCC_ID) break that.
static int placement_broken(ddrl_ctx* c) {
  if (!c->xcc_pending) return 0;
  int x[32] = {0};
  if (hipMemcpy(x, c->xcc, sizeof(x), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  const int per = 2 * c->xcc_ksp;   // workgroups per policy
  int bad = 0;
  for (int p = 0; p < 8; ++p) {
    if (!(c->xcc_mask & (1 << p))) continue;
    for (int j = 1; j < per && p + 8 * j < c->xcc_pending; ++j) bad |= x[p + 8 * j] != x[p];
  }
  c->xcc_pending = 0;
  return bad;
}

// The one-launch GNN step needs the 32 tiles of each (net, backward share) combination on one
// XCD (gnn.hip gnn_tail).  Returns 1 if the last such launch's per-tile XCC record breaks that.
static int gnn_placement_broken(ddrl_ctx* c) {
  if (c->cfg.model_kind != DDRL_MODEL_GNN || !c->gnn.xcc_pending) return 0;
  c->gnn.xcc_pending = 0;
  int x[256] = {0};
  if (hipMemcpy(x, c->gnn.xcc, sizeof(x), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  int bad = 0;
  for (int k = 0; k < 8; ++k)
    for (int t = 1; t < DDRL_MB / 4; ++t) bad |= x[32 * k + t] != x[32 * k];
  return bad;
}

// A failed peer launch may have left partly written outboxes on both ranks: the pair must
// re-attach (rank 0's attach clears them) before another peer update, or a retry's tag bit could
// admit the aborted launch's stale quads.  Detaching makes ddrl_ppo_update_peer
// refuse ("no peer") until ddrl_peer_attach runs again.
static void peer_detach(ddrl_ctx* c) {
  c->peer_gx = nullptr;
  c->peer_rank = -1;
  c->peer_inflight = 0;
}

static int check_err(ddrl_ctx* c) {
  int e = 0;
  HIPCHK(hipMemcpy(&e, c->err, sizeof(int), hipMemcpyDeviceToHost));
  const int was_peer = c->peer_inflight;
  c->peer_inflight = 0;
  if (e) {
    (void)hipMemset(c->err, 0, sizeof(int));
    const int bad = placement_broken(c);
    const int gbad = gnn_placement_broken(c);
    if (restore_snapshot(c)) return -1;
    c->snap_mask = 0;
    if (was_peer) {
      peer_detach(c);
      return fail("peer update: an exchange with the peer rank's launch was abandoned (3 s timeout or a failed "
                  "launch).  The weights, Adam state and beta powers are as before the call; this context is "
                  "detached from its peer: both ranks must call ddrl_peer_attach again before a peer update");
    }
    if (c->cfg.model_kind == DDRL_MODEL_GNN) {
      // a one-launch GNN step whose waits were abandoned or refused a flag from another XCD:
      // the context goes on with the three-launch step (no cross-workgroup waits)
      const int was_tail = c->gnn.tail && c->gnn.lists == 1;
      c->gnn.tail = 0;
      if (!was_tail)   // the three-launch step has no waits between workgroups
        return fail("GraphNet update: a launch reported an error (the error word was set).  The weights, Adam "
                    "state and beta powers are as before the call");
      return fail(std::string("GraphNet update: ") +
                  (gbad ? "the workgroups of a (net, backward share) combination ran on different XCDs (placement "
                          "check), so the one-launch step's reduction through the XCD's L2 was refused"
                        : "a wait between workgroups was abandoned (3 s timeout or a failed launch)") +
                  ".  The weights, Adam state and beta powers are as before the call; this context has switched "
                  "to the three-launch step: call the update again");
    }
    if (bad && !c->xchg_atomic) {
      c->xchg_atomic = 1;
      return fail("update kernel: the workgroups of a policy ran on different XCDs (placement check), so the "
                  "default exchange through the XCD's L2 could not complete.  The weights, Adam state and beta "
                  "powers are as before the call; this context has switched to the atomic exchange protocol "
                  "(valid for any placement): call the update again");
    }
    return fail("update kernel: an exchange between the workgroups of a policy was abandoned (3 s timeout or "
                "a failed launch).  The weights, Adam state and beta powers are as before the call");
  }
  // a broken placement whose exchanges still completed (a granule reached the other XCD through
  // memory) gave correct results -- the tags admit only this step's data -- but the next
  // launch might not be so lucky: switch protocols now
  if (placement_broken(c)) c->xchg_atomic = 1;
  // the GNN reducers accept flags only from their own XCD, so a step that completed had its
  // combinations in place; a record that says otherwise still ends the one-launch steps
  if (gnn_placement_broken(c)) c->gnn.tail = 0;
  c->snap_mask = 0;
  return 0;
}

// fcnet update launch with the context's exchange protocol
static void launch_ffn(ddrl_ctx* c, const UpdateArgs* ua, const UpdateHyper& h, int nrows, float inv_n, int d,
                       int stride, int ksp, int mask) {
  c->xcc_pending = ksp == 2 ? 24 + h.P : 8 + h.P;
  c->xcc_ksp = ksp;
  c->xcc_mask = mask;
  // test hook (DDRL_TEST_FAIL_STEP): a fused launch starts with the error word set, as an
  // exchange abandoned in its first step would leave it -- every workgroup runs its steps and
  // none writes back (no per-step cost in the kernel; a compare per step measured 0.18 us)
  if (c->fail_step >= 0 && !ua->grad_out) (void)hipMemsetD32Async((hipDeviceptr_t)c->err, 1, 1, c->stream);
  // a fused launch runs the kernels of the context's minibatch size; gradient-export launches
  // carry at most 128 rows at either size and run the 128-row kernels
  const bool mb256 = c->cfg.sgd_minibatch_size == 256 && !ua->grad_out;
  (mb256 ? (c->xchg_atomic ? launch_update_ffn_mb256_atomic : launch_update_ffn_mb256)
         : (c->xchg_atomic ? launch_update_ffn_atomic : launch_update_ffn))(
      c->stream, ua, h, nrows, inv_n, c->cfg.act_dim, d, stride, c->cfg.leg_coupling, c->xchg, c->gx, ksp, c->err,
      &c->upd_epoch, c->xcc, -1, 0u);
}

int ddrl_synchronize(ddrl_ctx* c) {
  CHK_CTX(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipGetLastError());
  return check_err(c);
}

int ddrl_param_count(ddrl_ctx* c, int pid, int64_t* n) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies || !n) return fail("bad policy id");
  *n = c->pol[pid].n_params;
  return 0;
}

int ddrl_record_layout(ddrl_ctx* c, int pid, int32_t* o) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies || !o) return fail("bad policy id");
  const RecLayout& L = c->pol[pid].lay;
  o[0] = L.stride; o[1] = L.obs; o[2] = L.act; o[3] = L.logit; o[4] = L.logp;
  o[5] = L.vf; o[6] = L.adv; o[7] = L.vt; o[8] = L.rew; o[9] = c->pol[pid].C; o[10] = L.cid;
  return 0;
}

static int check_n(ddrl_ctx* c, int pid, size_t n) {
  if (!c) return fail("null context");
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  if (n != (size_t)c->pol[pid].n_params) return fail("parameter count mismatch");
  return 0;
}

int ddrl_params_set(ddrl_ctx* c, int pid, const float* h, size_t n) {
  if (check_n(c, pid, n)) return -1;
  HIPCHK(hipMemcpyAsync(c->pol[pid].theta, h, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_params_get(ddrl_ctx* c, int pid, float* h, size_t n) {
  if (check_n(c, pid, n)) return -1;
  HIPCHK(hipMemcpyAsync(h, c->pol[pid].theta, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_adam_set(ddrl_ctx* c, int pid, const float* m, const float* v, size_t n, float b1p, float b2p) {
  if (check_n(c, pid, n)) return -1;
  Policy& P = c->pol[pid];
  HIPCHK(hipMemcpyAsync(P.m, m, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(P.v, v, n * 4, hipMemcpyHostToDevice, c->stream));
  float bp[2] = {b1p, b2p};
  HIPCHK(hipMemcpyAsync(P.beta_pow, bp, 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_adam_get(ddrl_ctx* c, int pid, float* m, float* v, size_t n, float* b1p, float* b2p) {
  if (check_n(c, pid, n)) return -1;
  Policy& P = c->pol[pid];
  float bp[2];
  HIPCHK(hipMemcpyAsync(m, P.m, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(v, P.v, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(bp, P.beta_pow, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (b1p) *b1p = bp[0];
  if (b2p) *b2p = bp[1];
  return 0;
}

int ddrl_filter_set(ddrl_ctx* c, double n, const double* M, const double* S) {
  CHK_CTX(c);
  const int D = c->cfg.obs_full_dim;
  HIPCHK(hipMemcpyAsync(c->f_n, &n, 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->f_M, M, D * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->f_S, S, D * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->ev_normc_ok = 0;
  c->sens_act_ok = 0;
  return 0;
}

int ddrl_filter_get(ddrl_ctx* c, double* n, double* M, double* S) {
  CHK_CTX(c);
  const int D = c->cfg.obs_full_dim;
  HIPCHK(hipMemcpyAsync(n, c->f_n, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(M, c->f_M, D * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(S, c->f_S, D * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_filter_delta_get(ddrl_ctx* c, double* n, double* M, double* S) {
  CHK_CTX(c);
  const int D = c->cfg.obs_full_dim;
  HIPCHK(hipMemcpyAsync(n, c->f_dn, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(M, c->f_dM, D * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(S, c->f_dS, D * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_filter_delta_reset(ddrl_ctx* c) {
  CHK_CTX(c);
  HIPCHK(hipMemsetAsync(c->f_dn, 0, 8, c->stream));
  HIPCHK(hipMemsetAsync(c->f_dM, 0, DDRL_MAXFULL * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->f_dS, 0, DDRL_MAXFULL * 8, c->stream));
  return 0;
}

static int pf_io(ddrl_ctx* c, int pid, double* n, double* M, double* S, bool set, bool delta) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  if (!n || !M || !S) return fail("null filter buffer");
  const int d = c->pol[pid].d;
  double* P = c->pf + (size_t)pid * PF_STRIDE;
  const int on = delta ? PF_DN : PF_N, om = delta ? PF_DM : PF_M, os = delta ? PF_DS : PF_S;
  const hipMemcpyKind k = set ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
  HIPCHK(hipMemcpyAsync(set ? (void*)(P + on) : (void*)n, set ? (const void*)n : (const void*)(P + on), 8, k, c->stream));
  HIPCHK(hipMemcpyAsync(set ? (void*)(P + om) : (void*)M, set ? (const void*)M : (const void*)(P + om), 8 * d, k, c->stream));
  HIPCHK(hipMemcpyAsync(set ? (void*)(P + os) : (void*)S, set ? (const void*)S : (const void*)(P + os), 8 * d, k, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (set) {   // normalization constants of the restored statistics
    launch_policy_filter(c->stream, c->route, nullptr, c->f_normc, 0.f, c->zs, c->pf, 0);
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return 0;
}

int ddrl_policy_filter_set(ddrl_ctx* c, int pid, double n, const double* M, const double* S) {
  return pf_io(c, pid, &n, const_cast<double*>(M), const_cast<double*>(S), true, false);
}
int ddrl_policy_filter_get(ddrl_ctx* c, int pid, double* n, double* M, double* S) {
  return pf_io(c, pid, n, M, S, false, false);
}
int ddrl_policy_filter_delta_get(ddrl_ctx* c, int pid, double* n, double* M, double* S) {
  return pf_io(c, pid, n, M, S, false, true);
}
int ddrl_policy_filter_delta_reset(ddrl_ctx* c) {
  CHK_CTX(c);
  for (int p = 0; p < c->cfg.n_policies; ++p) {
    double* P = c->pf + (size_t)p * PF_STRIDE;
    HIPCHK(hipMemsetAsync(P + PF_DN, 0, 8 * (1 + 2 * DDRL_MAXD), c->stream));
  }
  return 0;
}

int ddrl_adv_sums_get(ddrl_ctx* c, int pid, double* host3) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  const Policy& P = c->pol[pid];
  const size_t nblocks = (P.C + 255) / 256;
  HIPCHK(hipMemcpyAsync(host3, P.partials + 2 * nblocks, 3 * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// "cup" model: the leg-coupling table [4][A] follows the policy's fcnet variables (null: none)
static const float* cup_table(const ddrl_ctx* c, int p) {
  return c->cfg.leg_coupling ? c->pol[p].theta + ffn_param_count(c->pol[p].d, c->cfg.act_dim) : nullptr;
}

// the clip of the env-side filter as the kernels take it (0: none)
static float effective_clip(const ddrl_cfg& g) { return g.filter_enabled ? g.filter_clip : 0.f; }

// stream-ordered copy of a host env plane's pinned buffer
static int h2d(ddrl_ctx* c, void* dst, const void* src, size_t bytes) {
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream) == hipSuccess ? 0 : fail("H2D copy failed");
}

// what ddrl_eval_act and ddrl_eval_sens read of the context
static PolicyInputArgs make_policy_input(const ddrl_ctx* c, const float* obs) {
  PolicyInputArgs in{};
  for (int p = 0; p < c->cfg.n_policies; ++p) {
    in.theta[p] = c->pol[p].theta;
    in.cup[p] = cup_table(c, p);
  }
  in.obs = obs; in.normc = c->f_normc; in.pf = c->cfg.policy_filter ? c->pf : nullptr;
  in.clip = effective_clip(c->cfg);
  return in;
}

static int check_range(const ddrl_ctx* c, int e0, int e1) {
  if (e0 < 0 || e1 > c->cfg.n_envs || e0 >= e1) return fail("env range [e0, e1) must lie in [0, n_envs) and be non-empty");
  return 0;
}

// observe / act / reward over the envs [e0, e1) (the whole shard, or one group of a
// pipelined host env plane): the env-side filter pushes the range's rows as one batch.
int ddrl_observe_range(ddrl_ctx* c, const float* obs, int e0, int e1) {
  CHK_CTX(c);
  if (!obs) return fail("null observation buffer");
  if (check_range(c, e0, e1)) return -1;
  const ddrl_cfg& g = c->cfg;
  const int n = e1 - e0;
  const float* obs_r = obs + (size_t)e0 * g.obs_full_dim;
  RouteArgs ra = c->route;
  ra.N = n;
  ra.e0 = e0;
  c->ev_normc_ok = 0;
  c->sens_act_ok = 0;
  launch_filter_push(c->stream, obs_r, n, g.obs_full_dim, c->f_n, c->f_M, c->f_S, c->f_normc,
                     g.filter_update, g.filter_enabled, c->f_dn, c->f_dM, c->f_dS, c->f_part);
  const float clip = effective_clip(g);
  if (g.policy_filter) launch_policy_filter(c->stream, ra, obs_r, c->f_normc, clip, c->zs, c->pf, 1);
  const FilterCount fc{c->f_n, c->f_dn, g.filter_enabled && g.filter_update ? n : 0};
  if (g.model_kind == DDRL_MODEL_FFN)
    launch_observe_ffn(c->stream, ra, obs, c->f_normc, clip, c->stage_tab, g.policy_filter ? c->pf : nullptr, fc);
  else
    launch_observe_gnn(c->stream, ra, obs, c->f_normc, clip, c->pol[0].stage, fc);
  HIPCHK(hipGetLastError());
  return 0;
}

int ddrl_observe(ddrl_ctx* c, const float* obs) {
  CHK_CTX(c);
  return ddrl_observe_range(c, obs, 0, c->cfg.n_envs);
}

static ActArgs make_act(ddrl_ctx* c, int t, const float* eps, float* actions, int mode) {
  ActArgs aa{};
  for (int p = 0; p < c->cfg.n_policies; ++p) {
    Policy& P = c->pol[p];
    aa.theta[p] = P.theta; aa.stage[p] = P.stage; aa.rec[p] = P.rec; aa.last_v[p] = P.last_v;
    aa.lay[p] = P.lay; aa.C[p] = P.C;
    aa.cup[p] = cup_table(c, p);
  }
  aa.t = t; aa.eps = eps; aa.actions = actions; aa.bootstrap = mode;
  aa.e0 = 0; aa.e1 = c->cfg.n_envs;
  return aa;
}

static int launch_act(ddrl_ctx* c, const ActArgs& aa) {
  if (c->cfg.model_kind == DDRL_MODEL_FFN) launch_act_ffn(c->stream, c->route, aa);
  else launch_act_gnn(c->stream, c->route, aa, c->cfg.gnn_layer);
  HIPCHK(hipGetLastError());
  return 0;
}

int ddrl_act(ddrl_ctx* c, int t, const float* eps, float* actions) {
  CHK_CTX(c);
  if (t < 0 || t >= c->cfg.frag_len) return fail("t out of range");
  if (!eps || !actions) return fail("null eps/actions buffer");
  return launch_act(c, make_act(c, t, eps, actions, 0));
}

int ddrl_act_range(ddrl_ctx* c, int t, int e0, int e1, const float* eps, float* actions) {
  CHK_CTX(c);
  if (t < 0 || t >= c->cfg.frag_len) return fail("t out of range");
  if (!eps || !actions) return fail("null eps/actions buffer");
  if (check_range(c, e0, e1)) return -1;
  ActArgs aa = make_act(c, t, eps, actions, 0);
  aa.e0 = e0;
  aa.e1 = e1;
  return launch_act(c, aa);
}

int ddrl_bootstrap(ddrl_ctx* c) {
  CHK_CTX(c);
  return launch_act(c, make_act(c, 0, nullptr, nullptr, 1));
}

// the reward tables of the context (record pointers included; env range and t by the caller)
static RewardArgs make_reward(ddrl_ctx* c) {
  const ddrl_cfg& g = c->cfg;
  RewardArgs ra{};
  ra.P = g.n_policies; ra.N = g.n_envs; ra.n_agents = g.n_agents; ra.mode = g.reward_mode;
  ra.e0 = 0; ra.n = g.n_envs;
  ra.ctrl_w = g.ctrl_cost_weight; ra.contact_w = g.contact_cost_weight;
  for (int p = 0; p < g.n_policies; ++p) {
    ra.k[p] = c->pol[p].k; ra.rec[p] = c->pol[p].rec; ra.lay[p] = c->pol[p].lay;
    for (int s = 0; s < c->pol[p].k; ++s) {
      ra.policy_of_agent[c->pol[p].agents[s]] = p;
      ra.slot_of_agent[c->pol[p].agents[s]] = s;
    }
  }
  for (int j = 0; j < g.n_agents; ++j) {
    ra.n_act[j] = g.act_dim;
    for (int a = 0; a < 8; ++a) ra.act_index[j][a] = g.act_index[j][a];
    ra.n_contact[j] = g.n_contact[j];
    for (int b = 0; b < 14; ++b) {
      ra.contact_index[j][b] = g.contact_index[j][b];
      ra.contact_weight[j][b] = g.contact_weight[j][b];
    }
  }
  return ra;
}

int ddrl_reward(ddrl_ctx* c, int t, const float* fw, const float* cfrc, const float* actions,
                const uint8_t* done) {
  CHK_CTX(c);
  return ddrl_reward_range(c, t, 0, c->cfg.n_envs, fw, cfrc, actions, done);
}

int ddrl_reward_range(ddrl_ctx* c, int t, int e0, int e1, const float* fw, const float* cfrc, const float* actions,
                      const uint8_t* done) {
  CHK_CTX(c);
  if (t < 0 || t >= c->cfg.frag_len) return fail("t out of range");
  if (!fw || !cfrc || !actions) return fail("null reward input");
  if (check_range(c, e0, e1)) return -1;
  RewardArgs ra = make_reward(c);
  ra.e0 = e0; ra.n = e1 - e0;
  ra.t = t;
  c->ep_collected = 0;
  launch_reward(c->stream, ra, fw, cfrc, actions, done, c->done_tn);
  HIPCHK(hipGetLastError());
  return 0;
}

static int rollout_launches(ddrl_ctx* c, const float* obs, const float* eps, const float* fw, const float* cfrc,
                            const uint8_t* done, float* actions) {
  const ddrl_cfg& g = c->cfg;
  const size_t N = g.n_envs;
  for (int t = 0; t < g.frag_len; ++t) {
    if (ddrl_act(c, t, eps + (size_t)t * N * g.n_agents * g.act_dim, actions)) return -1;
    if (ddrl_reward(c, t, fw + (size_t)t * N, cfrc + (size_t)t * N * 14 * 6, actions, done ? done + (size_t)t * N : nullptr))
      return -1;
    if (ddrl_observe(c, obs + (size_t)(t + 1) * N * g.obs_full_dim)) return -1;
  }
  return ddrl_bootstrap(c);
}

int ddrl_rollout_fragment(ddrl_ctx* c, const float* obs, const float* eps, const float* fw, const float* cfrc,
                          const uint8_t* done, float* actions) {
  CHK_CTX(c);
  if (!obs || !eps || !fw || !cfrc || !actions) return fail("null rollout buffer");
  if (!c->rollout_graph) return rollout_launches(c, obs, eps, fw, cfrc, done, actions);
  const void* key[6] = {obs, eps, fw, cfrc, done, actions};
  if (!c->rg_exec || !std::equal(key, key + 6, c->rg_key)) {
    if (c->rg_exec) {
      HIPCHK(hipGraphExecDestroy(c->rg_exec));
      c->rg_exec = nullptr;
    }
    // captured on a private stream (a capture records, it does not run), launched on the caller's
    if (!c->cap_stream) HIPCHK(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
    const hipStream_t user = c->stream;
    c->stream = c->cap_stream;
    hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) {
      c->stream = user;
      return fail(std::string("rollout graph capture: ") + hipGetErrorString(e));
    }
    const int rc = rollout_launches(c, obs, eps, fw, cfrc, done, actions);
    hipGraph_t graph = nullptr;
    e = hipStreamEndCapture(c->stream, &graph);
    c->stream = user;
    if (rc) {
      if (graph) (void)hipGraphDestroy(graph);
      return -1;
    }
    if (e != hipSuccess) return fail(std::string("rollout graph capture: ") + hipGetErrorString(e));
    const hipError_t ei = hipGraphInstantiate(&c->rg_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) {
      c->rg_exec = nullptr;
      return fail(std::string("rollout graph instantiate: ") + hipGetErrorString(ei));
    }
    std::copy(key, key + 6, c->rg_key);
  }
  HIPCHK(hipGraphLaunch(c->rg_exec, c->stream));
  c->ep_collected = 0;
  return 0;
}

int ddrl_step_host(ddrl_ctx* c, int t, const float* obs_h, const float* eps_h, float* act_h) {
  CHK_CTX(c);
  const ddrl_cfg& g = c->cfg;
  HIPCHK(hipMemcpyAsync(c->h_obs, obs_h, (size_t)g.n_envs * g.obs_full_dim * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->h_eps, eps_h, (size_t)g.n_envs * g.n_agents * g.act_dim * 4, hipMemcpyHostToDevice,
                        c->stream));
  if (ddrl_observe(c, c->h_obs)) return -1;
  if (ddrl_act(c, t, c->h_eps, c->h_act)) return -1;
  HIPCHK(hipMemcpyAsync(act_h, c->h_act, (size_t)g.n_envs * 8 * 4, hipMemcpyDeviceToHost, c->stream));
  return 0;
}

int ddrl_act_host(ddrl_ctx* c, int t, const float* eps_h, float* act_h) {
  CHK_CTX(c);
  if (!eps_h || !act_h) return fail("null host buffer");
  const ddrl_cfg& g = c->cfg;
  HIPCHK(hipMemcpyAsync(c->h_eps, eps_h, (size_t)g.n_envs * g.n_agents * g.act_dim * 4, hipMemcpyHostToDevice,
                        c->stream));
  if (ddrl_act(c, t, c->h_eps, c->h_act)) return -1;
  HIPCHK(hipMemcpyAsync(act_h, c->h_act, (size_t)g.n_envs * 8 * 4, hipMemcpyDeviceToHost, c->stream));
  return 0;
}

int ddrl_env_step_host(ddrl_ctx* c, int t, const float* fw_h, const float* cfrc_h, const uint8_t* done_h,
                       const float* obs_h) {
  CHK_CTX(c);
  if (!fw_h || !cfrc_h || !obs_h) return fail("null host buffer");
  const ddrl_cfg& g = c->cfg;
  const size_t N = g.n_envs;
  HIPCHK(hipMemcpyAsync(c->h_fw, fw_h, N * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->h_cfrc, cfrc_h, N * 14 * 6 * 4, hipMemcpyHostToDevice, c->stream));
  if (done_h) HIPCHK(hipMemcpyAsync(c->h_done, done_h, N, hipMemcpyHostToDevice, c->stream));
  // the env actions of step t are still in h_act (act_host / step_host wrote them)
  if (ddrl_reward(c, t, c->h_fw, c->h_cfrc, c->h_act, done_h ? c->h_done : nullptr)) return -1;
  HIPCHK(hipMemcpyAsync(c->h_obs, obs_h, N * g.obs_full_dim * 4, hipMemcpyHostToDevice, c->stream));
  return ddrl_observe(c, c->h_obs);
}

// f1: a fragment with the envs stepped on the host (ddrl_hostenv, hostenv.cpp), pipelined over
// `groups` env groups: while the host threads step group g, the device runs the other groups'
// reward / observe / act and the transfers.  Per step t and group g (envs [e0, e1)):
//   wait for the actions of (t, g) (event) -> host step of [e0, e1) into the pinned buffers ->
//   H2D of the group's fw / cfrc / done / next obs -> reward_range(t) -> observe_range ->
//   act_range(t + 1) -> D2H of the group's actions -> event.
// The call order on the stream is the same as a synchronous loop over the same groups, so the
// records are bit-identical to it (tests/test_gpu_hostenv.py).  reset: 1 = reset every env
// first and observe the reset observations (per group); 0 = continue from the observation
// the context holds.  eps_dev: [T][N][n_agents][A] exploration noise in HBM.  Ends with the
// bootstrap V(s_T) of every env.
int ddrl_rollout_hostenv(ddrl_ctx* c, ddrl_hostenv* env, int groups, const float* eps_dev, int reset) {
  CHK_CTX(c);
  const ddrl_cfg& g = c->cfg;
  if (!env || !eps_dev) return fail("null host env / noise buffer");
  if (env->N != g.n_envs || env->D != g.obs_full_dim) return fail("host env shape differs from the context's");
  if (groups < 1 || groups > 8 || groups > g.n_envs) return fail("groups must be in [1, min(8, n_envs)]");
  const int N = g.n_envs, D = g.obs_full_dim, T = g.frag_len;
  const size_t eps_step = (size_t)N * g.n_agents * g.act_dim;
  std::vector<int> lo(groups + 1);
  for (int k = 0; k <= groups; ++k) lo[k] = (int)((long long)N * k / groups);
  std::vector<hipEvent_t> ev(groups, nullptr);
  for (auto& e : ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  int rc = 0;
  auto d2h_act = [&](int k) {
    const size_t off = (size_t)lo[k] * 8;
    if (hipMemcpyAsync(env->act + off, c->h_act + off, (size_t)(lo[k + 1] - lo[k]) * 8 * 4, hipMemcpyDeviceToHost,
                       c->stream) != hipSuccess || hipEventRecord(ev[k], c->stream) != hipSuccess)
      return fail("D2H copy failed");
    return 0;
  };
  if (reset) env->reset_all();
  for (int k = 0; k < groups && !rc; ++k) {
    const int e0 = lo[k], e1 = lo[k + 1];
    if (reset) rc = h2d(c, c->h_obs + (size_t)e0 * D, env->obs + (size_t)e0 * D, (size_t)(e1 - e0) * D * 4) ||
                    ddrl_observe_range(c, c->h_obs, e0, e1);
    rc = rc || ddrl_act_range(c, 0, e0, e1, eps_dev, c->h_act) || d2h_act(k);
  }
  for (int t = 0; t < T && !rc; ++t) {
    for (int k = 0; k < groups && !rc; ++k) {
      const int e0 = lo[k], e1 = lo[k + 1], n = e1 - e0;
      if (hipEventSynchronize(ev[k]) != hipSuccess) { rc = fail("event wait failed"); break; }
      env->step(e0, e1);   // host threads; the device meanwhile runs the other groups' work
      rc = h2d(c, c->h_fw + e0, env->fw + e0, (size_t)n * 4) ||
           h2d(c, c->h_cfrc + (size_t)e0 * 84, env->cfrc + (size_t)e0 * 84, (size_t)n * 84 * 4) ||
           h2d(c, c->h_done + e0, env->done + e0, (size_t)n) ||
           h2d(c, c->h_obs + (size_t)e0 * D, env->obs + (size_t)e0 * D, (size_t)n * D * 4) ||
           ddrl_reward_range(c, t, e0, e1, c->h_fw, c->h_cfrc, c->h_act, c->h_done) ||
           ddrl_observe_range(c, c->h_obs, e0, e1);
      if (!rc && t + 1 < T)
        rc = ddrl_act_range(c, t + 1, e0, e1, eps_dev + (size_t)(t + 1) * eps_step, c->h_act) || d2h_act(k);
    }
  }
  if (!rc) rc = ddrl_bootstrap(c);
  // the pinned buffers are the caller's again only once the stream has consumed them
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail("stream synchronize failed");
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc ? -1 : 0;
}

// ---- evaluation (eval.hip) -----------------------------------------------------------
// Whole episodes of the context's policies, N envs x E episodes each.  Nothing here writes a
// record, done_tn, last_v, a per-policy filter, Adam state or a parameter.
#define CHK_EVAL(c)                                    \
  do {                                                 \
    CHK_CTX(c);                                        \
    if (!(c)->ev_on) return fail("evaluation: call ddrl_eval_begin first"); \
  } while (0)

int ddrl_eval_begin(ddrl_ctx* c, const ddrl_eval_cfg* ec) {
  CHK_CTX(c);
  if (!ec) return fail("null evaluation config");
  if (c->cfg.model_kind != DDRL_MODEL_FFN) return fail("evaluation: fcnet models only");
  if (ec->episodes_per_env < 1) return fail("evaluation: episodes_per_env must be >= 1");
  if (ec->ctrl_roll < 0 || ec->ctrl_roll > 7) return fail("evaluation: ctrl_roll must be in [0, 7]");
  if (!(ec->total_mass > 0.0)) return fail("evaluation: total_mass must be > 0");
  const size_t N = c->cfg.n_envs, E = ec->episodes_per_env;
  HIPCHK(hipStreamSynchronize(c->stream));   // nothing in flight reads a table that is replaced
  if (!c->ev_acc) {
    if (dalloc(c, &c->ev_acc, N * 4) || dalloc(c, &c->ev_count, N) || dalloc(c, &c->ev_ctr, 2) ||
        dalloc(c, &c->ev_kin, N * 9))
      return -1;
  }
  if ((int)E > c->ev_table_E) {
    dfree(c, &c->ev_table);
    c->ev_table_E = 0;
    if (dalloc(c, &c->ev_table, N * E * 6)) return -1;
    c->ev_table_E = (int)E;
  }
  HIPCHK(hipMemsetAsync(c->ev_acc, 0, N * 4 * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->ev_count, 0, N * 4, c->stream));
  HIPCHK(hipMemsetAsync(c->ev_ctr, 0, 2 * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->ev_table, 0xFF, N * E * 6 * 8, c->stream));   // all-ones doubles: NaN rows
  c->ev_cfg = *ec;
  c->ev_normc_ok = 0;
  c->sens_on = 0;
  c->sens_act_ok = 0;
  c->mem_on = 0;
  c->ev_on = 1;
  return 0;
}

// ---- evaluation members (eval_members.hip) -------------------------------------------------
int ddrl_eval_members_begin(ddrl_ctx* c, int n_members) {
  CHK_EVAL(c);
  const ddrl_cfg& g = c->cfg;
  if (n_members < 1) return fail("evaluation members: n_members must be >= 1");
  if (g.n_envs % n_members) return fail("evaluation members: n_members must divide n_envs");
  if (c->sens_on) return fail("evaluation members: the sensitivity mode is on (sensitivity per member is not supported)");
  const int M = n_members, n = g.n_envs / M;
  HIPCHK(hipStreamSynchronize(c->stream));   // nothing in flight reads a buffer that is replaced
  c->mem_on = 0;
  if (M > c->mem_cap) {
    for (int p = 0; p < g.n_policies; ++p) dfree(c, &c->mem_theta[p]);
    dfree(c, &c->mem_filt);
    dfree(c, &c->mem_pf);
    c->mem_cap = 0;
    for (int p = 0; p < g.n_policies; ++p) {
      c->mem_tstride[p] = ((size_t)c->pol[p].n_params + 3) & ~(size_t)3;
      if (dalloc(c, &c->mem_theta[p], (size_t)M * c->mem_tstride[p])) return -1;
    }
    if (dalloc(c, &c->mem_filt, (size_t)M * FM_STRIDE) ||
        dalloc(c, &c->mem_pf, (size_t)M * g.n_policies * PF_STRIDE))
      return -1;
    c->mem_cap = M;
  }
  // the chunk scratch depends on n as well: M * filter_part_doubles(n) is largest at the smallest M
  dfree(c, &c->mem_part);
  if (dalloc(c, &c->mem_part, (size_t)M * filter_part_doubles(n, DDRL_MAXFULL))) return -1;
  c->mem_loaded.assign(M, 0);
  c->mem_normc_ok = 0;
  c->mem_on = M;
  return 0;
}

#define CHK_MEMBER(c, m)                                                                    \
  do {                                                                                      \
    CHK_EVAL(c);                                                                            \
    if (!(c)->mem_on) return fail("evaluation members: call ddrl_eval_members_begin first"); \
    if ((m) < 0 || (m) >= (c)->mem_on)                                                      \
      return fail("evaluation members: member " + std::to_string(m) + " is out of range [0, " + \
                  std::to_string((c)->mem_on) + ")");                                       \
  } while (0)

int ddrl_eval_member_load(ddrl_ctx* c, int member) {
  CHK_MEMBER(c, member);
  const ddrl_cfg& g = c->cfg;
  const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
  for (int p = 0; p < g.n_policies; ++p)
    HIPCHK(hipMemcpyAsync(c->mem_theta[p] + (size_t)member * c->mem_tstride[p], c->pol[p].theta,
                          (size_t)c->pol[p].n_params * 4, dd, c->stream));
  double* F = c->mem_filt + (size_t)member * FM_STRIDE;
  HIPCHK(hipMemcpyAsync(F + FM_N, c->f_n, 8, dd, c->stream));
  HIPCHK(hipMemcpyAsync(F + FM_M, c->f_M, DDRL_MAXFULL * 8, dd, c->stream));
  HIPCHK(hipMemcpyAsync(F + FM_S, c->f_S, DDRL_MAXFULL * 8, dd, c->stream));
  HIPCHK(hipMemsetAsync(F + FM_DN, 0, (1 + 2 * DDRL_MAXFULL) * 8, c->stream));   // the delta stat starts empty
  if (g.policy_filter) {
    // the constants ddrl_eval_act would use now: the read-only pass rewrites them from (n, M, S)
    launch_policy_filter(c->stream, c->route, nullptr, c->f_normc, 0.f, c->zs, c->pf, 0);
    HIPCHK(hipGetLastError());
    const size_t n = (size_t)g.n_policies * PF_STRIDE;
    HIPCHK(hipMemcpyAsync(c->mem_pf + (size_t)member * n, c->pf, n * 8, dd, c->stream));
  }
  c->mem_loaded[member] = 1;
  c->mem_normc_ok = 0;
  return 0;
}

int ddrl_eval_member_filter_get(ddrl_ctx* c, int member, double* n, double* M, double* S) {
  CHK_MEMBER(c, member);
  if (!n || !M || !S) return fail("null filter buffer");
  const int D = c->cfg.obs_full_dim;
  const double* F = c->mem_filt + (size_t)member * FM_STRIDE;
  HIPCHK(hipMemcpyAsync(n, F + FM_N, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(M, F + FM_M, D * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(S, F + FM_S, D * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// ddrl_eval_act with the member mode on: member state only, the context's own is not touched
static int eval_act_members(ddrl_ctx* c, const float* obs, const float* eps, float* actions,
                            float* const* logits_out) {
  const ddrl_cfg& g = c->cfg;
  const int M = c->mem_on, n = g.n_envs / M;
  for (int m = 0; m < M; ++m)
    if (!c->mem_loaded[m]) return fail("evaluation members: member " + std::to_string(m) + " has not been loaded");
  const int push = g.filter_enabled && c->ev_cfg.filter_update;
  // a frozen filter's constants are written once per members_begin / member_load
  if (push || !c->mem_normc_ok) {
    launch_filter_push_members(c->stream, obs, n, g.obs_full_dim, M, c->mem_filt, c->ev_cfg.filter_update,
                               g.filter_enabled, c->mem_part);
    c->mem_normc_ok = !push;
  }
  EvalMembersArgs ma{};
  for (int p = 0; p < g.n_policies; ++p) {
    ma.theta[p] = c->mem_theta[p];
    ma.theta_stride[p] = c->mem_tstride[p];
    ma.cup_off[p] = g.leg_coupling ? ffn_param_count(c->pol[p].d, g.act_dim) : -1;
    ma.logits_out[p] = logits_out ? logits_out[p] : nullptr;
  }
  ma.obs = obs; ma.filt = c->mem_filt;
  ma.pf = g.policy_filter ? c->mem_pf : nullptr;
  ma.pf_stride = (size_t)g.n_policies * PF_STRIDE;
  ma.clip = effective_clip(g);
  ma.eps = eps; ma.actions = actions;
  RouteArgs ra = c->route;
  ra.e0 = 0;
  ra.N = n;
  launch_eval_act_members(c->stream, ra, ma, M, push ? n : 0);
  HIPCHK(hipGetLastError());
  return 0;
}

int ddrl_eval_act(ddrl_ctx* c, const float* obs, const float* eps, float* actions, float* const* logits_out) {
  CHK_EVAL(c);
  if (!obs || !actions) return fail("null observation / actions buffer");
  if (c->mem_on) return eval_act_members(c, obs, eps, actions, logits_out);
  const ddrl_cfg& g = c->cfg;
  const int N = g.n_envs;
  const int push = g.filter_enabled && c->ev_cfg.filter_update;
  const float clip = effective_clip(g);
  // the normalization constants are rewritten only when a push changes them, or when this is
  // the first step since something else (eval_begin, filter_set, observe) may have
  if (push || !c->ev_normc_ok) {
    launch_filter_push(c->stream, obs, N, g.obs_full_dim, c->f_n, c->f_M, c->f_S, c->f_normc, c->ev_cfg.filter_update,
                       g.filter_enabled, c->f_dn, c->f_dM, c->f_dS, c->f_part);
    // RLlib compute_action filters with update=False: constants only, the statistics stay
    if (g.policy_filter) launch_policy_filter(c->stream, c->route, obs, c->f_normc, clip, c->zs, c->pf, 0);
    c->ev_normc_ok = !push;
  }
  EvalActArgs ea{};
  ea.in = make_policy_input(c, obs);
  for (int p = 0; p < g.n_policies; ++p) ea.logits_out[p] = logits_out ? logits_out[p] : nullptr;
  ea.eps = eps; ea.actions = actions;
  ea.fc = FilterCount{c->f_n, c->f_dn, push ? N : 0};
  RouteArgs ra = c->route;
  ra.e0 = 0;
  launch_eval_act(c->stream, ra, ea);
  HIPCHK(hipGetLastError());
  c->sens_act_ok = 1;
  return 0;
}

int ddrl_eval_step(ddrl_ctx* c, const float* fw, const float* cfrc, const float* actions, const float* kin,
                   const uint8_t* done) {
  CHK_EVAL(c);
  if (!fw || !cfrc || !actions || !kin || !done) return fail("null evaluation step input");
  RewardArgs ra = make_reward(c);
  for (int p = 0; p < DDRL_MAXP; ++p) ra.rec[p] = nullptr;   // the accumulator writes no record
  EvalAccumArgs ev{};
  ev.acc = c->ev_acc; ev.ep_count = c->ev_count; ev.table = c->ev_table; ev.counters = c->ev_ctr;
  ev.E = c->ev_cfg.episodes_per_env; ev.ctrl_roll = c->ev_cfg.ctrl_roll; ev.total_mass = c->ev_cfg.total_mass;
  launch_eval_accum(c->stream, ra, ev, fw, cfrc, actions, kin, done);
  HIPCHK(hipGetLastError());
  return 0;
}

int ddrl_eval_progress(ddrl_ctx* c, int64_t* episodes_done, int64_t* envs_finished) {
  CHK_EVAL(c);
  if (!episodes_done || !envs_finished) return fail("null progress output");
  unsigned long long ctr[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(ctr, c->ev_ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipGetLastError());
  if (check_err(c)) return -1;
  *episodes_done = (int64_t)ctr[0];
  *envs_finished = (int64_t)ctr[1];
  return 0;
}

int ddrl_eval_results(ddrl_ctx* c, double* host, size_t n_rows) {
  CHK_EVAL(c);
  if (!host) return fail("null results buffer");
  const size_t rows = (size_t)c->cfg.n_envs * c->ev_cfg.episodes_per_env;
  if (n_rows != rows) return fail("evaluation: the result table has n_envs * episodes_per_env rows");
  HIPCHK(hipMemcpyAsync(host, c->ev_table, rows * 6 * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_eval_end(ddrl_ctx* c) {
  CHK_EVAL(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  c->ev_on = 0;
  c->sens_on = 0;
  c->mem_on = 0;
  return 0;
}

// ---- input sensitivity (eval_sens.hip) ---------------------------------------------------
int ddrl_eval_sens_begin(ddrl_ctx* c, const double* const* step_host) {
  CHK_EVAL(c);
  if (c->cfg.model_kind != DDRL_MODEL_FFN) return fail("sensitivity: fcnet models only");
  if (c->mem_on) return fail("sensitivity: the evaluation member mode is on (sensitivity per member is not supported)");
  if (!step_host) return fail("sensitivity: null step array");
  const ddrl_cfg& g = c->cfg;
  std::vector<double> steps((size_t)DDRL_MAXP * DDRL_MAXD, 0.0);
  for (int p = 0; p < g.n_policies; ++p) {
    if (!step_host[p]) return fail("sensitivity: null step array");
    for (int f = 0; f < c->pol[p].d; ++f) {
      const double h = step_host[p][f];
      if (!(h >= 0.0) || !(h <= 1.7976931348623157e308)) return fail("sensitivity: steps must be finite and >= 0");
      steps[(size_t)p * DDRL_MAXD + f] = h;
    }
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if ((!c->sens_step && dalloc(c, &c->sens_step, steps.size())) ||
      (!c->sens_red && dalloc(c, &c->sens_red, 2 * DDRL_MAXD * 8 + 1)))
    return -1;
  for (int p = 0; p < g.n_policies; ++p) {
    const Policy& P = c->pol[p];
    if ((!c->sens_acc[p] && dalloc(c, &c->sens_acc[p], (size_t)P.C * 2 * P.d * g.act_dim)) ||
        (!c->sens_cnt[p] && dalloc(c, &c->sens_cnt[p], P.C)))
      return -1;
  }
  HIPCHK(hipMemcpyAsync(c->sens_step, steps.data(), steps.size() * 8, hipMemcpyHostToDevice, c->stream));
  for (int p = 0; p < g.n_policies; ++p) {
    const Policy& P = c->pol[p];
    HIPCHK(hipMemsetAsync(c->sens_acc[p], 0, (size_t)P.C * 2 * P.d * g.act_dim * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->sens_cnt[p], 0, (size_t)P.C * 8, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));   // `steps` is read until here
  c->sens_on = 1;
  return 0;
}

#define CHK_SENS(c)                                    \
  do {                                                 \
    CHK_EVAL(c);                                       \
    if (!(c)->sens_on) return fail("sensitivity: call ddrl_eval_sens_begin first"); \
  } while (0)

int ddrl_eval_sens(ddrl_ctx* c, const float* obs, float* const* means_out) {
  CHK_SENS(c);
  if (!obs) return fail("null observation buffer");
  if (!c->sens_act_ok)
    return fail("sensitivity: call ddrl_eval_act on this observation first (the filter constants may have changed)");
  const ddrl_cfg& g = c->cfg;
  EvalSensArgs sa{};
  sa.in = make_policy_input(c, obs);
  for (int p = 0; p < g.n_policies; ++p) {
    sa.means_out[p] = means_out ? means_out[p] : nullptr;
    sa.acc[p] = c->sens_acc[p];
    sa.rowcnt[p] = c->sens_cnt[p];
  }
  sa.step = c->sens_step; sa.ep_count = c->ev_count; sa.E = c->ev_cfg.episodes_per_env;
  // one base row per workgroup up to 512 rows per policy, a loop over base rows past that (the
  // measured choice, DESIGN.md "Sensitivity"); DDRL_SENS_GRID (read at every launch) moves the cap
  int cap = 512;
  if (const char* e = std::getenv("DDRL_SENS_GRID")) cap = std::max(1, std::atoi(e));
  RouteArgs ra = c->route;
  ra.e0 = 0;
  launch_eval_sens(c->stream, ra, sa, cap);
  HIPCHK(hipGetLastError());
  return 0;
}

int ddrl_eval_sens_results(ddrl_ctx* c, int policy, double* grads, double* grads_abs, int64_t* rows) {
  CHK_SENS(c);
  if (policy < 0 || policy >= c->cfg.n_policies) return fail("bad policy id");
  if (!grads || !grads_abs || !rows) return fail("null sensitivity output");
  const Policy& P = c->pol[policy];
  const int n = P.d * c->cfg.act_dim;
  long long* rows_dev = reinterpret_cast<long long*>(c->sens_red + 2 * DDRL_MAXD * 8);
  launch_sens_reduce(c->stream, c->sens_acc[policy], c->sens_cnt[policy], P.C, 2 * n, c->sens_red, rows_dev);
  HIPCHK(hipGetLastError());
  long long r = 0;
  HIPCHK(hipMemcpyAsync(grads, c->sens_red, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(grads_abs, c->sens_red + n, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&r, rows_dev, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *rows = (int64_t)r;
  return 0;
}

int ddrl_eval_hostenv(ddrl_ctx* c, ddrl_hostenv* env, const float* eps_dev, int eps_steps, int max_steps,
                      int poll_every, int* steps_run) {
  CHK_EVAL(c);
  const ddrl_cfg& g = c->cfg;
  if (!env) return fail("null host env");
  if (c->mem_on)
    return fail("evaluation: the member mode is on and the host env plane has no per-env target velocity "
                "(use the device env plane)");
  if (env->N != g.n_envs || env->D != g.obs_full_dim) return fail("host env shape differs from the context's");
  if (max_steps < 1 || poll_every < 1) return fail("evaluation: max_steps and poll_every must be >= 1");
  if (eps_dev && eps_steps < 1) return fail("evaluation: eps_steps must be >= 1 with a noise buffer");
  const size_t N = g.n_envs, D = g.obs_full_dim;
  const size_t eps_step = N * g.n_agents * g.act_dim;
  const int limit = eps_dev ? std::min(max_steps, eps_steps) : max_steps;
  env->reset_episodes();
  int rc = h2d(c, c->h_obs, env->obs, N * D * 4);
  int t = 0;
  for (; t < limit && !rc;) {
    rc = ddrl_eval_act(c, c->h_obs, eps_dev ? eps_dev + (size_t)t * eps_step : nullptr, c->h_act, nullptr);
    if (!rc && c->sens_on) rc = ddrl_eval_sens(c, c->h_obs, nullptr);
    if (!rc && hipMemcpyAsync(env->act, c->h_act, N * 8 * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
      rc = fail("D2H copy failed");
    // the actions are on the host, and the previous step's H2D copies have left the pinned buffers
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail("stream synchronize failed");
    if (rc) break;
    env->step(0, (int)N);
    rc = h2d(c, c->h_fw, env->fw, N * 4) || h2d(c, c->h_cfrc, env->cfrc, N * 84 * 4) || h2d(c, c->h_done, env->done, N) ||
         h2d(c, c->ev_kin, env->kin, N * 9 * 4) || h2d(c, c->h_obs, env->obs, N * D * 4) ||
         ddrl_eval_step(c, c->h_fw, c->h_cfrc, c->h_act, c->ev_kin, c->h_done);
    ++t;
    if (!rc && t % poll_every == 0) {
      int64_t eps_done = 0, fin = 0;
      rc = ddrl_eval_progress(c, &eps_done, &fin);
      if (!rc && fin == (int64_t)N) break;
    }
  }
  // the pinned buffers are the caller's again only once the stream has consumed them
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail("stream synchronize failed");
  if (steps_run) *steps_run = t;
  return rc ? -1 : 0;
}

// ---- device env plane (devenv.hip) --------------------------------------------------------
static int chk_env(const ddrl_devenv* e) {
  if (!e) return fail("null device env");
  if (!e->ctx) return fail("device env: its context has been destroyed");
  return 0;
}
#define CHK_ENV(e) \
  if (chk_env(e)) return -1

// The terrain settings into the kernel arguments.  A captured fragment has them baked into its
// step nodes, so a change that a terrain launch would see (before or after it) re-keys the graph;
// flat to flat (new_terrain on flat ground) changes nothing a flat launch reads.
static void devenv_put_terrain(ddrl_devenv* e, const envdyn::Terrain& t) {
  DevEnvArgs& a = e->a;
  const int was_on = a.ter_on;
  a.ter_lo = t.lo; a.ter_hi = t.hi; a.ter_bump = t.bump_scale; a.ter_inv_bump = t.inv_bump; a.ter_gen = t.generation;
  a.ter_on = envdyn::terrain_on(t) ? 1 : 0;
  if (was_on || a.ter_on) ++e->gen;
}

int ddrl_devenv_create(ddrl_ctx* c, uint64_t seed, float target_velocity, ddrl_devenv** out) {
  CHK_CTX(c);
  if (!out) return fail("ddrl_devenv_create: null output pointer");
  const ddrl_cfg& g = c->cfg;
  if (g.obs_full_dim != 43 && g.obs_full_dim != 44)
    return fail("ddrl_devenv_create: the context's obs_full_dim must be 43 or 44");
  if (g.obs_full_dim == 44 && !(target_velocity > 0.f))
    return fail("ddrl_devenv_create: obs_full_dim 44 needs target_velocity > 0");
  HIPCHK(hipSetDevice(c->device));   // the buffers live on the context's device
  static std::atomic<uint64_t> next_id{0};
  auto* e = new ddrl_devenv();
  e->ctx = c;
  e->id = ++next_id;
  const size_t N = g.n_envs;
  DevEnvArgs& a = e->a;
  a.N = g.n_envs; a.D = g.obs_full_dim; a.time_limit = 1000; a.n_tv = 1; a.seed = seed;
  devenv_put_terrain(e, envdyn::terrain_flat());
  e->tv_cap = 16;
  e->tv_list.assign(1, (double)target_velocity);
  // the create-time velocity until the first reset draws one, as the host plane
  const std::vector<double> tv0(N, (double)target_velocity);
  const bool ok = env_alloc(e, &a.st, (size_t)DDRL_DEVENV_FIELDS * N) && env_alloc(e, &a.steps, N) && env_alloc(e, &a.episode, N) &&
                  env_alloc(e, &e->tv_dev, e->tv_cap) && env_alloc(e, &a.obs, N * a.D) && env_alloc(e, &a.fw, N) && env_alloc(e, &a.cfrc, N * 84) &&
                  env_alloc(e, &a.kin, N * 9) && env_alloc(e, &a.done, N) && env_alloc(e, &e->packed, N * DDRL_ENV_STATE_DOUBLES) &&
                  hipMemcpy(a.st + 38 * N, tv0.data(), N * 8, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(e->tv_dev, e->tv_list.data(), 8, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    for (void* p : e->allocs) (void)hipFree(p);
    delete e;
    return fail("ddrl_devenv_create: device buffer allocation failed");
  }
  a.tv_list = e->tv_dev;
  c->devenvs.push_back(e);
  *out = e;
  return 0;
}

int ddrl_devenv_destroy(ddrl_devenv* e) {
  if (!e) return 0;
  if (ddrl_ctx* c = e->ctx) {
    (void)hipStreamSynchronize(c->stream);   // nothing in flight touches the buffers
    c->devenvs.erase(std::remove(c->devenvs.begin(), c->devenvs.end(), e), c->devenvs.end());
  }
  for (void* p : e->allocs) (void)hipFree(p);
  delete e;
  return 0;
}

int ddrl_devenv_buffers(ddrl_devenv* e, float** obs, float** fw, float** cfrc, float** kin, uint8_t** done) {
  CHK_ENV(e);
  if (obs) *obs = e->a.obs;
  if (fw) *fw = e->a.fw;
  if (cfrc) *cfrc = e->a.cfrc;
  if (kin) *kin = e->a.kin;
  if (done) *done = e->a.done;
  return 0;
}

static int devenv_reset(ddrl_devenv* e, int mode) {
  CHK_ENV(e);
  launch_devenv_reset(e->ctx->stream, e->a, mode);
  HIPCHK(hipGetLastError());
  return 0;
}
int ddrl_devenv_reset(ddrl_devenv* e) { return devenv_reset(e, DEVENV_RESET_ALL); }
int ddrl_devenv_reset_episodes(ddrl_devenv* e) { return devenv_reset(e, DEVENV_RESET_EPISODES); }
int ddrl_devenv_reset_state(ddrl_devenv* e) { return devenv_reset(e, DEVENV_RESET_STATE); }

int ddrl_devenv_set_time_limit(ddrl_devenv* e, int steps) {
  CHK_ENV(e);
  if (steps < 1) return fail("ddrl_devenv_set_time_limit: steps >= 1");
  e->a.time_limit = steps;
  ++e->gen;
  return 0;
}

int ddrl_devenv_set_target_velocities(ddrl_devenv* e, const float* list, int n) {
  CHK_ENV(e);
  if (!list || n < 1) return fail("ddrl_devenv_set_target_velocities: a list of n >= 1 values");
  for (int i = 0; i < n; ++i) {
    if (!std::isfinite(list[i])) return fail("ddrl_devenv_set_target_velocities: target velocities must be finite");
    if (e->a.D > 43 && !(list[i] > 0.f))
      return fail("ddrl_devenv_set_target_velocities: obs_dim 44 needs target velocities > 0 "
                  "(the TVel reward divides by it)");
  }
  // launches in flight still read the old list
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  if ((size_t)n > e->tv_cap) {
    double* p = nullptr;
    HIPCHK(hipMalloc((void**)&p, (size_t)n * 8));
    e->allocs.push_back(p);   // the smaller list is freed with the env
    e->tv_dev = p;
    e->tv_cap = n;
  }
  e->tv_list.assign(list, list + n);
  HIPCHK(hipMemcpy(e->tv_dev, e->tv_list.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  e->a.tv_list = e->tv_dev;
  e->a.n_tv = n;
  ++e->gen;
  return 0;
}

int ddrl_devenv_set_env_target_velocities(ddrl_devenv* e, const float* per_env, int n_envs) {
  CHK_ENV(e);
  if (per_env) {
    if (n_envs != e->a.N) return fail("ddrl_devenv_set_env_target_velocities: per_env holds n_envs floats");
    for (int i = 0; i < n_envs; ++i) {
      if (!std::isfinite(per_env[i]))
        return fail("ddrl_devenv_set_env_target_velocities: target velocities must be finite");
      if (e->a.D > 43 && !(per_env[i] > 0.f))
        return fail("ddrl_devenv_set_env_target_velocities: obs_dim 44 needs target velocities > 0 "
                    "(the TVel reward divides by it)");
    }
  }
  // launches in flight still read the old table
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  if (per_env) {
    if (!e->tv_env_dev && !env_alloc(e, &e->tv_env_dev, (size_t)e->a.N))
      return fail("ddrl_devenv_set_env_target_velocities: device buffer allocation failed");
    const std::vector<double> tv(per_env, per_env + n_envs);
    HIPCHK(hipMemcpy(e->tv_env_dev, tv.data(), (size_t)n_envs * 8, hipMemcpyHostToDevice));
    e->a.tv_env = e->tv_env_dev;
  } else {
    e->a.tv_env = nullptr;
  }
  ++e->gen;
  return 0;
}

int ddrl_devenv_target_velocities(ddrl_devenv* e, float* out, int n) {
  CHK_ENV(e);
  if (!out || n != e->a.N) return fail("ddrl_devenv_target_velocities: out holds n_envs floats");
  std::vector<double> tv(n);
  HIPCHK(hipMemcpyAsync(tv.data(), e->a.st + (size_t)38 * n, (size_t)n * 8, hipMemcpyDeviceToHost, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  for (int i = 0; i < n; ++i) out[i] = (float)tv[i];
  return 0;
}

int ddrl_devenv_set_terrain(ddrl_devenv* e, double lo, double hi, double bump_scale, uint32_t generation) {
  CHK_ENV(e);
  if (!(0.0 <= lo && lo <= hi && hi <= 1.0))
    return fail("ddrl_devenv_set_terrain: smoothness bounds must satisfy 0 <= lo <= hi <= 1");
  if (!(bump_scale > 0.0) || !std::isfinite(bump_scale))
    return fail("ddrl_devenv_set_terrain: bump_scale must be a finite value > 0");
  // launches already issued hold their own copy of the arguments: no synchronization
  devenv_put_terrain(e, envdyn::Terrain{lo, hi, bump_scale, 1.0 / bump_scale, generation});
  return 0;
}

int ddrl_devenv_terrain(ddrl_devenv* e, double* lo, double* hi, double* bump_scale, uint32_t* generation) {
  CHK_ENV(e);
  if (lo) *lo = e->a.ter_lo;
  if (hi) *hi = e->a.ter_hi;
  if (bump_scale) *bump_scale = e->a.ter_bump;
  if (generation) *generation = e->a.ter_gen;
  return 0;
}

int ddrl_devenv_new_terrain(ddrl_devenv* e) {
  CHK_ENV(e);
  devenv_put_terrain(e, envdyn::Terrain{e->a.ter_lo, e->a.ter_hi, e->a.ter_bump, e->a.ter_inv_bump, e->a.ter_gen + 1u});
  return 0;
}

int ddrl_devenv_terrain_height(ddrl_devenv* e, const int32_t* env_index_dev, const double* xy_dev, int n,
                               double* out_dev) {
  CHK_ENV(e);
  if (!env_index_dev || !xy_dev || !out_dev || n < 0)
    return fail("ddrl_devenv_terrain_height: n >= 0 points (env_index[n], xy[n][2]) and out[n] in device memory");
  launch_devenv_terrain_height(e->ctx->stream, e->a, env_index_dev, xy_dev, n, out_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ddrl_devenv_step(ddrl_devenv* e, const float* actions) {
  CHK_ENV(e);
  if (!actions) return fail("ddrl_devenv_step: null actions buffer");
  launch_devenv_step(e->ctx->stream, e->a, actions);
  HIPCHK(hipGetLastError());
  return 0;
}

int ddrl_devenv_state_get(ddrl_devenv* e, double* host, size_t n) {
  CHK_ENV(e);
  if (!host || n != (size_t)e->a.N * DDRL_ENV_STATE_DOUBLES)
    return fail("ddrl_devenv_state_get: n == n_envs * DDRL_ENV_STATE_DOUBLES doubles");
  launch_devenv_pack(e->ctx->stream, e->a, e->packed, 0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(host, e->packed, n * 8, hipMemcpyDeviceToHost, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  return 0;
}

int ddrl_devenv_state_set(ddrl_devenv* e, const double* host, size_t n) {
  CHK_ENV(e);
  if (!host || n != (size_t)e->a.N * DDRL_ENV_STATE_DOUBLES)
    return fail("ddrl_devenv_state_set: n == n_envs * DDRL_ENV_STATE_DOUBLES doubles");
  for (int i = 0; i < e->a.N; ++i)
    if (!envdyn::packed_counts_ok(host + (size_t)i * DDRL_ENV_STATE_DOUBLES))
      return fail("ddrl_devenv_state_set: steps and episode must be non-negative integers");
  HIPCHK(hipMemcpyAsync(e->packed, host, n * 8, hipMemcpyHostToDevice, e->ctx->stream));
  launch_devenv_pack(e->ctx->stream, e->a, e->packed, 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->ctx->stream));   // `host` is read until here
  return 0;
}

static int chk_env_of(const ddrl_ctx* c, const ddrl_devenv* e) {
  if (chk_env(e)) return -1;
  if (e->ctx != c) return fail("device env belongs to another context");
  return 0;
}

// act(t) -> env step -> reward(t) -> observe for every t, then the bootstrap: one linear chain
static int devenv_launches(ddrl_ctx* c, ddrl_devenv* e, const float* eps) {
  const ddrl_cfg& g = c->cfg;
  const size_t eps_step = (size_t)g.n_envs * g.n_agents * g.act_dim;
  for (int t = 0; t < g.frag_len; ++t) {
    if (ddrl_act(c, t, eps + (size_t)t * eps_step, c->h_act) || ddrl_devenv_step(e, c->h_act) ||
        ddrl_reward(c, t, e->a.fw, e->a.cfrc, c->h_act, e->a.done) || ddrl_observe(c, e->a.obs))
      return -1;
  }
  return ddrl_bootstrap(c);
}

int ddrl_rollout_devenv(ddrl_ctx* c, ddrl_devenv* e, const float* eps_dev, int reset) {
  CHK_CTX(c);
  if (chk_env_of(c, e)) return -1;
  if (!eps_dev) return fail("null noise buffer");
  if (reset && (ddrl_devenv_reset(e) || ddrl_observe(c, e->a.obs))) return -1;
  if (!c->rollout_graph) return devenv_launches(c, e, eps_dev);
  if (!c->rgd_exec || c->rgd_env != e->id || c->rgd_gen != e->gen || c->rgd_eps != eps_dev) {
    if (c->rgd_exec) {
      HIPCHK(hipGraphExecDestroy(c->rgd_exec));
      c->rgd_exec = nullptr;
    }
    // captured on a private stream (a capture records, it does not run), launched on the caller's
    if (!c->cap_stream) HIPCHK(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
    const hipStream_t user = c->stream;
    c->stream = c->cap_stream;
    hipError_t er = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
    if (er != hipSuccess) {
      c->stream = user;
      return fail(std::string("rollout graph capture: ") + hipGetErrorString(er));
    }
    const int rc = devenv_launches(c, e, eps_dev);
    hipGraph_t graph = nullptr;
    er = hipStreamEndCapture(c->stream, &graph);
    c->stream = user;
    if (rc) {
      if (graph) (void)hipGraphDestroy(graph);
      return -1;
    }
    if (er != hipSuccess) return fail(std::string("rollout graph capture: ") + hipGetErrorString(er));
    const hipError_t ei = hipGraphInstantiate(&c->rgd_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) {
      c->rgd_exec = nullptr;
      return fail(std::string("rollout graph instantiate: ") + hipGetErrorString(ei));
    }
    c->rgd_env = e->id; c->rgd_gen = e->gen; c->rgd_eps = eps_dev;
  }
  HIPCHK(hipGraphLaunch(c->rgd_exec, c->stream));
  // what the replayed calls would have noted on the host
  c->ep_collected = 0;
  c->ev_normc_ok = 0;
  c->sens_act_ok = 0;
  return 0;
}

int ddrl_eval_devenv(ddrl_ctx* c, ddrl_devenv* e, const float* eps_dev, int eps_steps, int max_steps, int poll_every,
                     int* steps_run) {
  CHK_EVAL(c);
  if (chk_env_of(c, e)) return -1;
  const ddrl_cfg& g = c->cfg;
  if (max_steps < 1 || poll_every < 1) return fail("evaluation: max_steps and poll_every must be >= 1");
  if (eps_dev && eps_steps < 1) return fail("evaluation: eps_steps must be >= 1 with a noise buffer");
  const size_t N = g.n_envs;
  const size_t eps_step = N * g.n_agents * g.act_dim;
  const int limit = eps_dev ? std::min(max_steps, eps_steps) : max_steps;
  int rc = ddrl_devenv_reset_episodes(e);
  int t = 0;
  for (; t < limit && !rc;) {
    rc = ddrl_eval_act(c, e->a.obs, eps_dev ? eps_dev + (size_t)t * eps_step : nullptr, c->h_act, nullptr);
    if (!rc && c->sens_on) rc = ddrl_eval_sens(c, e->a.obs, nullptr);
    rc = rc || ddrl_devenv_step(e, c->h_act) || ddrl_eval_step(c, e->a.fw, e->a.cfrc, c->h_act, e->a.kin, e->a.done);
    if (rc) break;
    ++t;
    if (t % poll_every == 0) {
      int64_t eps_done = 0, fin = 0;
      rc = ddrl_eval_progress(c, &eps_done, &fin);
      if (!rc && fin == (int64_t)N) break;
    }
  }
  if (steps_run) *steps_run = t;
  return rc ? -1 : 0;
}

// ---- episode accounting of the training rollout (episodes.hip) ---------------------------
// Nothing here writes a record, done_tn, last_v, a filter, Adam state or a parameter.
static int ep_state(ddrl_ctx* c) {
  if (c->ep_total) return 0;
  const size_t N = c->cfg.n_envs, TW = (size_t)c->cfg.frag_len * ((N + 63) / 64);
  return dalloc(c, &c->ep_total, N) || dalloc(c, &c->ep_agent, N * DDRL_MAXAG) || dalloc(c, &c->ep_len, N) ||
         dalloc(c, &c->ep_cnt, TW) || dalloc(c, &c->ep_base, TW) || dalloc(c, &c->ep_word, 1);
}

int ddrl_episodes_collect(ddrl_ctx* c, int64_t* n_finished) {
  CHK_CTX(c);
  if (!n_finished) return fail("episodes: null count output");
  if (c->ep_collected)
    return fail("episodes: this fragment has been collected (collect once per fragment, after its last reward)");
  if (ep_state(c)) return -1;
  const ddrl_cfg& g = c->cfg;
  const RewardArgs ra = make_reward(c);
  EpArgs a{};
  for (int p = 0; p < g.n_policies; ++p) { a.rec[p] = ra.rec[p]; a.lay[p] = ra.lay[p]; a.k[p] = ra.k[p]; }
  for (int j = 0; j < g.n_agents; ++j) {
    a.policy_of_agent[j] = ra.policy_of_agent[j];
    a.slot_of_agent[j] = ra.slot_of_agent[j];
  }
  a.N = g.n_envs; a.T = g.frag_len; a.n_agents = g.n_agents; a.W = (g.n_envs + 63) / 64;
  a.done_tn = c->done_tn; a.cnt = c->ep_cnt; a.base = c->ep_base; a.total = c->ep_word;
  a.ep_total = c->ep_total; a.ep_agent = c->ep_agent; a.ep_len = c->ep_len;
  launch_ep_count_scan(c->stream, a);
  HIPCHK(hipGetLastError());
  long long total = 0;
  HIPCHK(hipMemcpyAsync(&total, c->ep_word, sizeof(total), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));   // the one synchronize: nothing in flight reads the table either
  if (total < 0 || total > (long long)g.frag_len * g.n_envs) return fail("episodes: bad episode count");
  if (total > c->ep_cap) {
    const long long cap = std::max(total, 2 * c->ep_cap);
    dfree(c, &c->ep_table);
    c->ep_cap = 0;
    c->ep_rows = -1;
    if (dalloc(c, &c->ep_table, (size_t)cap * 8)) return -1;
    c->ep_cap = cap;
  }
  a.table = c->ep_table; a.cap = c->ep_cap;
  launch_ep_walk(c->stream, a);
  HIPCHK(hipGetLastError());
  c->ep_collected = 1;
  c->ep_rows = total;
  *n_finished = (int64_t)total;
  return 0;
}

int ddrl_episodes_rows(ddrl_ctx* c, double* host, size_t n_rows) {
  CHK_CTX(c);
  if (!host) return fail("episodes: null rows buffer");
  if (c->ep_rows < 0) return fail("episodes: call ddrl_episodes_collect first");
  if (n_rows != (size_t)c->ep_rows) return fail("episodes: n_rows differs from the last collect's count");
  if (n_rows) HIPCHK(hipMemcpyAsync(host, c->ep_table, n_rows * 8 * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_episodes_inflight(ddrl_ctx* c, double* host, size_t n_envs) {
  CHK_CTX(c);
  if (!host) return fail("episodes: null in-flight buffer");
  const size_t N = c->cfg.n_envs;
  if (n_envs != N) return fail("episodes: the in-flight state has n_envs rows");
  if (ep_state(c)) return -1;
  std::vector<double> tot(N), ag(N * DDRL_MAXAG);
  std::vector<int> len(N);
  HIPCHK(hipMemcpyAsync(tot.data(), c->ep_total, N * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(ag.data(), c->ep_agent, N * DDRL_MAXAG * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(len.data(), c->ep_len, N * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (size_t e = 0; e < N; ++e) {
    host[e * 6] = tot[e];
    for (int j = 0; j < DDRL_MAXAG; ++j) host[e * 6 + 1 + j] = ag[e * DDRL_MAXAG + j];
    host[e * 6 + 5] = (double)len[e];
  }
  return 0;
}

int ddrl_episodes_reset(ddrl_ctx* c) {
  CHK_CTX(c);
  if (!c->ep_total) return 0;   // nothing in flight yet
  const size_t N = c->cfg.n_envs;
  HIPCHK(hipMemsetAsync(c->ep_total, 0, N * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->ep_agent, 0, N * DDRL_MAXAG * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->ep_len, 0, N * 4, c->stream));
  return 0;
}

int ddrl_gae(ddrl_ctx* c) {
  CHK_CTX(c);
  const ddrl_cfg& g = c->cfg;
  GaeBatch gb{};
  gb.P = g.n_policies;
  for (int p = 0; p < g.n_policies; ++p) {
    Policy& P = c->pol[p];
    GaeArgs& ga = gb.g[p];
    ga.rec = P.rec; ga.lay = P.lay; ga.C = P.C; ga.T = g.frag_len; ga.N = g.n_envs; ga.k = P.k;
    ga.last_v = P.last_v; ga.done_tn = c->done_tn; ga.gamma = g.gamma; ga.lambda_ = g.lambda_;
    ga.partials = P.partials; ga.adv_norm = P.adv_norm;
  }
  launch_gae(c->stream, gb);
  HIPCHK(hipGetLastError());
  return 0;
}

static UpdateHyper make_hyper(ddrl_ctx* c, int P) {
  const ddrl_cfg& g = c->cfg;
  UpdateHyper h{};
  h.clip = g.clip_param; h.vf_clip = g.vf_clip_param; h.vf_coeff = g.vf_loss_coeff;
  h.ent_coeff = g.entropy_coeff; h.lr = g.lr; h.grad_clip = g.grad_clip; h.b1 = g.adam_beta1;
  h.b2 = g.adam_beta2; h.eps = g.adam_eps; h.vf_mode = g.vf_clip_mode; h.P = P;
  return h;
}

static UpdateArgs make_update(ddrl_ctx* c, int p, const int32_t* shuffle, const int32_t* perm, float kl) {
  Policy& P = c->pol[p];
  UpdateArgs u{};
  u.rec = P.rec; u.lay = P.lay; u.d = P.d; u.A = c->cfg.act_dim; u.R = P.R;
  u.shuffle = shuffle; u.perm = perm; u.nb = P.nb; u.n_epochs = c->cfg.num_sgd_iter;
  u.max_steps = -1; u.step0 = 0;
  u.theta = P.theta; u.m = P.m; u.v = P.v; u.beta_pow = P.beta_pow; u.stats = P.stats;
  u.adv_norm = P.adv_norm; u.grad_out = nullptr; u.gscr = P.grad; u.kl_coeff = kl;
  u.cup = c->cfg.leg_coupling;
  return u;
}

int ddrl_ppo_update(ddrl_ctx* c, int mask, const int32_t* const* shuffle, const int32_t* const* perm,
                    const float* kl, int max_steps) {
  return ddrl_ppo_update_from(c, mask, shuffle, perm, kl, 0, max_steps);
}

int ddrl_ppo_update_from(ddrl_ctx* c, int mask, const int32_t* const* shuffle, const int32_t* const* perm,
                         const float* kl, int step0, int max_steps) {
  CHK_CTX(c);
  if (!shuffle || !perm || !kl) return fail("null update argument");
  if (step0 < 0) return fail("step0 must be >= 0");
  UpdateArgs ua[DDRL_MAXP];
  int n = 0;
  for (int p = 0; p < c->cfg.n_policies; ++p) {
    if (!(mask & (1 << p))) continue;
    if (!shuffle[p] || !perm[p]) return fail("null shuffle/perm for a masked policy");
    // every minibatch is a full slice of the shuffled batch (RLlib's multi-GPU loader refuses
    // a batch smaller than one minibatch too); the kernels read shuffle[0 .. nb * sgd_minibatch_size)
    if (c->pol[p].R < c->cfg.sgd_minibatch_size)
      return fail("policy " + std::to_string(p) + ": the train batch holds " + std::to_string(c->pol[p].R) +
                  " rows, fewer than one minibatch (sgd_minibatch_size " +
                  std::to_string(c->cfg.sgd_minibatch_size) + ")");
    ua[n] = make_update(c, p, shuffle[p], perm[p], kl[p]);
    c->kl_last[p] = kl[p];
    ua[n].max_steps = max_steps;
    ua[n].step0 = step0;
    const int total = c->cfg.num_sgd_iter * c->pol[p].nb;
    if (step0 > total) return fail("step0 beyond the schedule's " + std::to_string(total) + " steps");
    c->pol[p].last_steps = max_steps >= 0 ? std::min(total - step0, max_steps) : total - step0;
    ++n;
  }
  if (n == 0) return 0;
  int maxd = 0, maxs = 0;  // KS1 instance / staging rows must cover the widest policy
  for (int i = 0; i < n; ++i) maxd = std::max(maxd, ua[i].d), maxs = std::max(maxs, ua[i].lay.stride);
  UpdateHyper h = make_hyper(c, n);
  // the arguments travel by value in the kernel's argument block (no copy from this stack frame)
  if (c->cfg.model_kind == DDRL_MODEL_FFN) {
    if (snapshot(c, mask & ((1 << c->cfg.n_policies) - 1))) return -1;
    launch_ffn(c, ua, h, c->cfg.sgd_minibatch_size, 1.f / c->cfg.sgd_minibatch_size, maxd, maxs, c->update_split,
               (1 << n) - 1);
  }
  else if (c->pol[0].last_steps > 0) {   // one shared policy
    const int last = c->pol[0].last_steps;
    if (!c->gnn.chunk && dalloc(c, &c->gnn.chunk, (size_t)c->gnn.chunk_steps * DDRL_MB * c->pol[0].lay.stride))
      return -1;
    if (snapshot(c, 1)) return -1;
    // test hook (DDRL_TEST_FAIL_STEP): the update starts with the error word set, as a failed
    // launch would leave it; the steps run, check_err restores the snapshot
    if (c->fail_step >= 0) (void)hipMemsetD32Async((hipDeviceptr_t)c->err, 1, 1, c->stream);
    const int CH = c->gnn.chunk_steps;
    // the records of each run of GNN_CHUNK_STEPS steps are gathered into one contiguous
    // chunk first (stream order: after the previous run's last step), so every gradient
    // launch reads its minibatch without dependent index loads
    const size_t step_floats = (size_t)DDRL_MB * ua[0].lay.stride;
    for (int step = step0; step < step0 + last; ++step) {
      const int k = (step - step0) % CH;
      if (k == 0) launch_gnn_gather(c->stream, ua[0], step, std::min(CH, step0 + last - step), c->gnn.chunk);
      launch_step_gnn(c->stream, ua[0], h, step, 128, 1.f / c->cfg.sgd_minibatch_size, c->gnn,
                      c->gnn.chunk + k * step_floats, c->cfg.gnn_layer);
    }
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int ddrl_ppo_stats(ddrl_ctx* c, int pid, float* host, size_t n_steps) {
  return ddrl_ppo_stats_range(c, pid, 0, n_steps, host);
}

int ddrl_ppo_stats_range(ddrl_ctx* c, int pid, size_t first, size_t n_steps, float* host) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  if (!host && n_steps) return fail("null stats buffer");
  const size_t cap = c->pol[pid].stats_steps;
  if (first > cap || n_steps > cap - first) return fail("more stats requested than the schedule holds");
  HIPCHK(hipMemcpyAsync(host, c->pol[pid].stats + first * 8, n_steps * 8 * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (check_err(c)) return -1;
  // the policy / value workgroups each write their own columns; total_loss is their
  // linear combination: mean(-surr) + beta*mean(kl) + vf_coeff*mean(vf) - ent_coeff*mean(H)
  const ddrl_cfg& g = c->cfg;
  const float beta = c->kl_last[pid];
  for (size_t k = 0; k < n_steps; ++k) {
    float* s = host + 8 * k;
    s[0] = s[1] + beta * s[3] + g.vf_loss_coeff * s[2] - g.entropy_coeff * s[4];
  }
  return 0;
}

// Grow policy pid's learner-statistics buffer to at least `rows` rows, keeping its contents.  A
// data-parallel loop in "split" mode runs 128 / (128 / G) = G times the fused schedule's
// minibatches per epoch, which passes the buffer sized at create (num_sgd_iter x R / 128 rows)
// when G > num_sgd_iter (found by the world-4 rehearsal with one epoch, round 6).  Growing waits
// for the context's stream; it happens once per size.
static int stats_reserve(ddrl_ctx* c, int pid, size_t rows) {
  Policy& P = c->pol[pid];
  if (rows <= P.stats_steps) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  float* nw = nullptr;
  if (dalloc(c, &nw, rows * 8)) return -1;
  if (P.stats_steps) HIPCHK(hipMemcpy(nw, P.stats, P.stats_steps * 8 * sizeof(float), hipMemcpyDeviceToDevice));
  dfree(c, &P.stats);
  P.stats = nw;
  P.stats_steps = rows;
  return 0;
}

// Workgroups per branch of a gradient-only update launch: the row split of the fused update
// when the rows fill both halves (64 each), else one.  ddrl_ppo_grad and ddrl_ppo_update_ddp
// share this rule, so the two data-parallel loops run the same kernels.
static int grad_split(const ddrl_ctx* c, int n_rows) { return n_rows > 64 ? c->update_split : 1; }

int ddrl_ppo_grad(ddrl_ctx* c, int pid, const int32_t* rows, int n_rows, float kl, float* grad,
                  int stats_step) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  if (n_rows < 1 || n_rows > 128) return fail("n_rows must be in [1, 128]");
  if (!rows || !grad) return fail("null rows/grad");
  if (stats_step >= 0 && (size_t)stats_step >= c->pol[pid].stats_steps &&
      stats_reserve(c, pid, std::max((size_t)stats_step + 1, 2 * c->pol[pid].stats_steps)))
    return -1;
  UpdateArgs u = make_update(c, pid, rows, c->zero_perm, kl);
  u.nb = 1; u.n_epochs = 1; u.max_steps = 1; u.step0 = 0; u.grad_out = grad;
  c->snap_mask = 0;   // a gradient launch changes no state: the caller's loop keeps its own snapshot
  u.stats = stats_step >= 0 ? c->pol[pid].stats + (size_t)stats_step * 8 : nullptr;
  c->kl_last[pid] = kl;
  UpdateHyper h = make_hyper(c, 1);
  if (c->cfg.model_kind == DDRL_MODEL_FFN)
    launch_ffn(c, &u, h, n_rows, 1.f / c->cfg.sgd_minibatch_size, c->pol[pid].d, c->pol[pid].lay.stride,
               grad_split(c, n_rows), 1);
  else
    launch_step_gnn(c->stream, u, h, 0, n_rows, 1.f / c->cfg.sgd_minibatch_size, c->gnn, nullptr, c->cfg.gnn_layer);
  HIPCHK(hipGetLastError());
  return 0;
}

int ddrl_ppo_apply(ddrl_ctx* c, int pid, const float* grad) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  if (!grad) return fail("null grad");
  Policy& P = c->pol[pid];
  launch_apply_adam(c->stream, grad, P.n_params, P.theta, P.m, P.v, P.beta_pow, make_hyper(c, 1), 1.f, pid, c->err);
  HIPCHK(hipGetLastError());
  return 0;
}

static_assert(sizeof(ncclUniqueId) == DDRL_COMM_ID_BYTES, "RCCL unique id size");

int ddrl_comm_unique_id(void* out, size_t n) {
  if (!out || n < sizeof(ncclUniqueId)) return fail("unique id buffer too small");
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  std::memcpy(out, &id, sizeof(id));
  return 0;
}

int ddrl_comm_init(ddrl_ctx* c, const void* id, int rank, int nranks) {
  CHK_CTX(c);
  if (!id || nranks < 1 || rank < 0 || rank >= nranks) return fail("bad communicator arguments");
  if (c->comm) return fail("the context already has a communicator");
  HIPCHK(hipSetDevice(c->device));
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  NCCLCHK(ncclCommInitRank(&c->comm, nranks, uid, rank));
  return 0;
}

int ddrl_comm_allreduce(ddrl_ctx* c, float* buf, size_t n) {
  CHK_CTX(c);
  if (!c->comm) return fail("no communicator (ddrl_comm_init)");
  if (!buf) return fail("null buffer");
  NCCLCHK(ncclAllReduce(buf, buf, n, ncclFloat32, ncclSum, c->comm, c->stream));
  return 0;
}

int ddrl_ppo_update_ddp(ddrl_ctx* c, int pid, const int32_t* shuffle, const int32_t* perm, int E, int nb,
                        int m, float kl, float gscale) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  if (!c->comm) return fail("no communicator (ddrl_comm_init)");
  if (!shuffle || !perm || E < 1 || nb < 1) return fail("bad schedule");
  // (sgd_minibatch_size 256: the split over two or more ranks fits, a whole minibatch per rank does not)
  if (m < 1 || m > 128) return fail("rows_per_rank must be in [1, 128]");
  if (stats_reserve(c, pid, (size_t)nb)) return -1;   // the last epoch's rows
  Policy& P = c->pol[pid];
  const int steps = E * nb;
  const UpdateHyper h = make_hyper(c, 1);
  const float inv_n = 1.f / c->cfg.sgd_minibatch_size;
  std::vector<UpdateArgs> ua((size_t)steps);
  for (int e = 0; e < E; ++e)
    for (int b = 0; b < nb; ++b) {
      const int slot = perm[(size_t)e * nb + b];
      if (slot < 0 || (size_t)(slot + 1) * m > (size_t)P.R) return fail("minibatch slot out of range");
      UpdateArgs u = make_update(c, pid, shuffle + (size_t)slot * m, c->zero_perm, kl);
      u.nb = 1; u.n_epochs = 1; u.max_steps = 1; u.step0 = 0; u.grad_out = P.grad;
      u.stats = e == E - 1 ? P.stats + (size_t)b * 8 : nullptr;
      ua[(size_t)e * nb + b] = u;
    }
  const bool ffn = c->cfg.model_kind == DDRL_MODEL_FFN;
  // the records of each run of up to DDP_CHUNK_STEPS steps are gathered into one contiguous
  // chunk first (stream order: after the previous run's last gradient launch), so a one-step
  // gradient launch stages its rows without the dependent perm -> shuffle index loads
  constexpr int DDP_CHUNK_STEPS = 1024;
  const int CH = std::min(DDP_CHUNK_STEPS, steps);
  const int stride = P.lay.stride;
  const size_t need = (size_t)CH * m * stride;
  // grown buffers replace the old ones (the previous call ended with a stream synchronize)
  if (c->ddp_chunk_n < need) {
    dfree(c, &c->ddp_chunk);
    c->ddp_chunk_n = 0;
    if (dalloc(c, &c->ddp_chunk, need)) return -1;
    c->ddp_chunk_n = need;
  }
  if (c->ddp_slots_n < (size_t)steps) {
    dfree(c, &c->ddp_slots);
    c->ddp_slots_n = 0;
    if (dalloc(c, &c->ddp_slots, (size_t)steps)) return -1;
    c->ddp_slots_n = (size_t)steps;
  }
  c->ddp_slots_host.assign(perm, perm + steps);
  HIPCHK(hipMemcpyAsync(c->ddp_slots, c->ddp_slots_host.data(), sizeof(int32_t) * steps, hipMemcpyHostToDevice,
                        c->stream));
  c->kl_last[pid] = kl;
  // restored by check_err if any step fails (the GNN gradient launches of 128 rows per rank
  // reduce in their tail, with bounded waits: ADVICE r4)
  if (snapshot(c, 1 << pid)) return -1;
  for (int s = 0; s < steps; ++s) {
    const int k = s % CH;
    if (k == 0) launch_rows_gather(c->stream, P.rec, stride, shuffle, c->ddp_slots, m, s, std::min(CH, steps - s),
                                   c->ddp_chunk);
    float* rows = c->ddp_chunk + (size_t)k * m * stride;
    // test hook: step s's gradient is lost (its Adam launch and every later one skip)
    if (s == c->fail_step) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)c->err, 1, 1, c->stream));
    if (ffn) {
      ua[s].rec = rows;
      ua[s].shuffle = nullptr;   // rows 0 .. m of the slice
      launch_ffn(c, &ua[s], h, m, inv_n, P.d, stride, grad_split(c, m), 1);
    } else {
      launch_step_gnn(c->stream, ua[s], h, 0, m, inv_n, c->gnn, rows, c->cfg.gnn_layer);
    }
    NCCLCHK(ncclAllReduce(P.grad, P.grad, (size_t)P.n_params, ncclFloat32, ncclSum, c->comm, c->stream));
    launch_apply_adam(c->stream, P.grad, P.n_params, P.theta, P.m, P.v, P.beta_pow, h, gscale, pid, c->err);
  }
  // every rank fails together: a norm-exchange timeout on one rank (whose zeroed gradient has
  // already been summed into every rank's weights) is all-reduced (max) into every rank's
  // error word, so no rank goes on to its next collective while another one raises
  NCCLCHK(ncclAllReduce(c->err, c->err, 1, ncclInt32, ncclMax, c->comm, c->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));   // the error word of every step
  return check_err(c);
}

static_assert(sizeof(hipIpcMemHandle_t) == DDRL_PEER_HANDLE_BYTES, "IPC handle size");

int ddrl_peer_alloc(ddrl_ctx* c, void** gx_out, void* ipc_handle_out) {
  CHK_CTX(c);
  if (!gx_out) return fail("null outbox pointer");
  HIPCHK(hipSetDevice(c->device));
  const size_t bytes = gx_bytes(DDRL_MAXP);
  void* p = nullptr;
  HIPCHK(hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained));
  c->allocs.push_back(p);
  HIPCHK(hipMemset(p, 0, bytes));
  if (ipc_handle_out) {
    hipIpcMemHandle_t h;
    HIPCHK(hipIpcGetMemHandle(&h, p));
    std::memcpy(ipc_handle_out, &h, sizeof(h));
  }
  *gx_out = p;
  return 0;
}

int ddrl_peer_open(ddrl_ctx* c, const void* ipc_handle, void** gx_out) {
  CHK_CTX(c);
  if (!ipc_handle || !gx_out) return fail("null IPC handle / outbox pointer");
  if (c->peer_ipc) return fail("the context already maps a peer's outboxes");
  HIPCHK(hipSetDevice(c->device));
  hipIpcMemHandle_t h;
  std::memcpy(&h, ipc_handle, sizeof(h));
  void* p = nullptr;
  HIPCHK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
  c->peer_ipc = p;
  *gx_out = p;
  return 0;
}

// Peer-mode buffers for E epochs of nb minibatch slots of policy pid: the statistics rows (the
// union batch has twice this rank's minibatches) and the virtual 128-row shuffle.  Growing them
// frees and allocates, which waits for the whole device -- for a peer context in the same
// process, whose launch waits for this one's, that is a stall until the 3 s bound -- so
// ddrl_peer_attach reserves the configured schedule (num_sgd_iter epochs of R / 64 slots) up front.
static int peer_reserve(ddrl_ctx* c, int pid, size_t E, size_t nb) {
  Policy& P = c->pol[pid];
  if (E * nb > P.stats_steps) {
    HIPCHK(hipStreamSynchronize(c->stream));
    dfree(c, &P.stats);
    P.stats_steps = 0;
    if (dalloc(c, &P.stats, E * nb * 8)) return -1;
    P.stats_steps = E * nb;
  }
  if (c->peer_vsh_n < nb * DDRL_MB) {
    HIPCHK(hipStreamSynchronize(c->stream));
    dfree(c, &c->peer_vsh);
    c->peer_vsh_n = 0;
    if (dalloc(c, &c->peer_vsh, nb * DDRL_MB)) return -1;
    c->peer_vsh_n = nb * DDRL_MB;
  }
  return 0;
}

int ddrl_peer_attach(ddrl_ctx* c, void* gx, int rank, int nranks) {
  CHK_CTX(c);
  if (!gx) return fail("null outboxes");
  if (nranks != 2 || rank < 0 || rank > 1) return fail("peer mode splits the minibatch over exactly two ranks");
  if (c->cfg.model_kind != DDRL_MODEL_FFN) return fail("peer mode is built for fcnet policies");
  if (c->update_split != 2) return fail("peer mode needs the row split (DDRL_UPDATE_SPLIT=2, the default)");
  if (c->cfg.sgd_minibatch_size != DDRL_MB)
    return fail("peer mode is built for sgd_minibatch_size 128 (64 rows per rank); this context has " +
                std::to_string(c->cfg.sgd_minibatch_size));
  // rank 0 clears the outboxes (no launch of either rank may be in flight: after a failed update
  // both ranks have synchronized; rank 1 attaches after rank 0); both count launches from here
  if (rank == 0) HIPCHK(hipMemsetAsync(gx, 0, gx_bytes(DDRL_MAXP), c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int p = 0; p < c->cfg.n_policies; ++p)
    if (peer_reserve(c, p, (size_t)c->cfg.num_sgd_iter, (size_t)c->pol[p].R / (DDRL_MB / 2))) return -1;
  c->peer_gx = gx;
  c->peer_rank = rank;
  c->peer_epoch = 0;
  c->peer_steps = 0;
  return 0;
}

int ddrl_ppo_update_peer(ddrl_ctx* c, int pid, const int32_t* shuffle, const int32_t* perm, int E, int nb, float kl,
                         int max_steps) {
  CHK_CTX(c);
  if (!c->peer_gx) return fail("no peer (ddrl_peer_attach)");
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  if (!shuffle || !perm || E < 1 || nb < 1) return fail("bad schedule");
  Policy& P = c->pol[pid];
  if ((size_t)nb * (DDRL_MB / 2) > (size_t)P.R) return fail("nb x 64 rows exceed this rank's train batch");
  if (peer_reserve(c, pid, (size_t)E, (size_t)nb)) return -1;   // no-op within the attached schedule
  // this rank's rows fill half peer_rank of every 128-row block of the shuffle the kernel indexes
  // (UpdateArgs::shuffle[slot * 128 + row], row half kq = rows 64 kq .. 64 kq + 63)
  constexpr int H = DDRL_MB / 2;
  HIPCHK(hipMemcpy2DAsync(c->peer_vsh + H * c->peer_rank, DDRL_MB * sizeof(int32_t), shuffle, H * sizeof(int32_t),
                          H * sizeof(int32_t), nb, hipMemcpyDeviceToDevice, c->stream));
  UpdateArgs u = make_update(c, pid, c->peer_vsh, perm, kl);
  u.nb = nb;
  u.n_epochs = E;
  u.max_steps = max_steps;
  const int total = E * nb;
  P.last_steps = max_steps >= 0 ? std::min(total, max_steps) : total;
  c->kl_last[pid] = kl;
  if (snapshot(c, 1 << pid)) return -1;
  c->xcc_pending = 0;   // the atomic protocol is valid for any placement
  UpdateHyper h = make_hyper(c, 1);
  launch_update_ffn_peer(c->stream, &u, h, DDRL_MB, 1.f / c->cfg.sgd_minibatch_size, c->cfg.act_dim, P.d,
                         P.lay.stride, c->cfg.leg_coupling, c->xchg, static_cast<unsigned long long*>(c->peer_gx), 2,
                         c->err, &c->peer_epoch, c->xcc, c->peer_rank, c->peer_steps);
  c->peer_steps += (unsigned)P.last_steps;   // the same count on both ranks
  c->peer_inflight = 1;
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) {
    peer_detach(c);
    return fail(std::string("peer update launch refused: ") + hipGetErrorString(le) +
                "; this context is detached from its peer (both ranks re-attach)");
  }
  return 0;
}

int ddrl_gnn_one_launch(ddrl_ctx* c, int* on) {
  CHK_CTX(c);
  if (!on) return fail("null output");
  *on = c->cfg.model_kind == DDRL_MODEL_GNN && c->gnn.tail && c->gnn.lists == 1;
  return 0;
}

int ddrl_policy_forward(ddrl_ctx* c, int pid, const float* obs, const int32_t* node, int n,
                        float* logits, float* values) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  if (n < 1 || !obs || !logits || !values) return fail("bad forward arguments");
  if (c->cfg.model_kind == DDRL_MODEL_GNN && !node) return fail("gnn forward needs the node index of every row");
  if (c->cfg.leg_coupling && !node) return fail("the \"cup\" forward needs the leg index of every row");
  Policy& P = c->pol[pid];
  ForwardArgs fa{};
  fa.theta = P.theta; fa.x = obs; fa.node = node; fa.n = n; fa.d = P.d; fa.A = c->cfg.act_dim;
  fa.logits = logits; fa.values = values;
  fa.cup = cup_table(c, pid);
  if (c->cfg.model_kind == DDRL_MODEL_FFN) launch_forward_ffn(c->stream, fa);
  else launch_forward_gnn(c->stream, fa, c->cfg.gnn_layer);
  HIPCHK(hipGetLastError());
  return 0;
}

int ddrl_records_get(ddrl_ctx* c, int pid, float* host, size_t n) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  const Policy& P = c->pol[pid];
  if (n != (size_t)P.R * P.lay.stride) return fail("record buffer size mismatch");
  HIPCHK(hipMemcpyAsync(host, P.rec, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_records_set(ddrl_ctx* c, int pid, const float* host, size_t n) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  const Policy& P = c->pol[pid];
  if (n != (size_t)P.R * P.lay.stride) return fail("record buffer size mismatch");
  HIPCHK(hipMemcpyAsync(P.rec, host, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->ep_collected = 0;
  return 0;
}

int ddrl_adv_norm_get(ddrl_ctx* c, int pid, float* host2) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  HIPCHK(hipMemcpyAsync(host2, c->pol[pid].adv_norm, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_adv_norm_set(ddrl_ctx* c, int pid, float mean, float den) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  float a[2] = {mean, den};
  HIPCHK(hipMemcpyAsync(c->pol[pid].adv_norm, a, 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_last_values_get(ddrl_ctx* c, int pid, float* host, size_t n) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  if (n != (size_t)c->pol[pid].C) return fail("last value count mismatch");
  HIPCHK(hipMemcpyAsync(host, c->pol[pid].last_v, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_last_values_set(ddrl_ctx* c, int pid, const float* host, size_t n) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  if (n != (size_t)c->pol[pid].C) return fail("last value count mismatch");
  HIPCHK(hipMemcpyAsync(c->pol[pid].last_v, host, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_done_set(ddrl_ctx* c, const uint8_t* host, size_t n) {
  CHK_CTX(c);
  if (n != (size_t)c->cfg.frag_len * c->cfg.n_envs) return fail("done buffer size mismatch");
  HIPCHK(hipMemcpyAsync(c->done_tn, host, n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_device_buffers(ddrl_ctx* c, int pid, void** records, void** last_v, void** params, void** adv_norm) {
  CHK_CTX(c);
  if (pid < 0 || pid >= c->cfg.n_policies) return fail("bad policy id");
  Policy& P = c->pol[pid];
  if (records) *records = P.rec;
  if (last_v) *last_v = P.last_v;
  if (params) *params = P.theta;
  if (adv_norm) *adv_norm = P.adv_norm;
  return 0;
}

}  // extern "C"

// ---- what the two groups of contexts (update, rollout) share; `kind` is "update" or "rollout" ----
namespace {
// A group's device table of per-member kernel arguments, rebuilt at every run in a pinned host array and copied on
// the group's stream.  That array is the source of the copy: host() waits for `copied`, recorded behind the copy.
template <class T>
struct MemberTable {
  T *pinned = nullptr, *dev = nullptr;
  hipEvent_t copied = nullptr;
  int copy_pending = 0;
  bool alloc(size_t n) {
    const size_t bytes = n * sizeof(T);
    return hipHostMalloc((void**)&pinned, bytes, hipHostMallocDefault) == hipSuccess && hipMalloc((void**)&dev, bytes) == hipSuccess &&
           hipMemset(dev, 0, bytes) == hipSuccess && hipEventCreateWithFlags(&copied, hipEventDisableTiming) == hipSuccess;
  }
  int host(T*& out) {
    if (copy_pending) HIPCHK(hipEventSynchronize(copied));
    copy_pending = 0;
    out = pinned;
    return 0;
  }
  int upload(hipStream_t stream, size_t n) {
    HIPCHK(hipMemcpyAsync(dev, pinned, n * sizeof(T), hipMemcpyHostToDevice, stream));
    HIPCHK(hipEventRecord(copied, stream));
    copy_pending = 1;
    return 0;
  }
  void stream_synced() { copy_pending = 0; }   // the caller has synchronized the stream of the last upload
  void release() {
    if (copied) (void)hipEventDestroy(copied);
    if (pinned) (void)hipHostFree(pinned);
    if (dev) (void)hipFree(dev);
  }
};

std::string group_member_name(const char* kind, int m) { return std::string(kind) + " group: member " + std::to_string(m); }

// create: no null and no repeated member (nor device env, where the group has them: envs != nullptr)
int group_list_ok(const char* kind, ddrl_ctx* const* members, ddrl_devenv* const* envs, int n_members) {
  for (int m = 0; m < n_members; ++m) {
    const std::string name = group_member_name(kind, m);
    if (!members[m]) return fail(name + " is a null context");
    if (envs && !envs[m]) return fail(name + " has a null device env");
    for (int k = 0; k < m; ++k) {
      if (members[k] == members[m]) return fail(name + " repeats member " + std::to_string(k));
      if (envs && envs[k] == envs[m]) return fail(name + " repeats the device env of member " + std::to_string(k));
    }
  }
  return 0;
}

// create: member m is an fcnet context on the group's device
int group_member_kind(const char* kind, const ddrl_ctx* c, int device, int m) {
  if (c->device != device) return fail(group_member_name(kind, m) + " is on another device than member 0");
  if (c->cfg.model_kind != DDRL_MODEL_FFN)
    return fail(group_member_name(kind, m) + " is a GraphNet context: the group " + kind + " runs the fcnet kernels only");
  return 0;
}

// same-shape checks: `why` names the first difference from member 0, found field by field (x.f against y.f)
#define DDRL_GRP_SAME(f) if (!why && !(x.f == y.f)) why = #f
int group_same_result(const char* kind, int m, const char* why) {
  return why ? fail(group_member_name(kind, m) + " differs from member 0 in " + why + ": a group takes contexts of one shape") : 0;
}
}  // namespace

// ---- group update (ppo_ffn_group.hip): the fused updates of M same-shaped contexts in one launch ----
// Chain g = m * P + p is policy p of member m.  The launches of a run hold whole members, in member
// order; launch l covers the chains [g0_l, g0_l + n_l) of the table and records its blocks' XCC ids
// at xcc + (sum of the earlier launches' grids).  The arenas (norm granules, outboxes) are sized for
// one launch's chains and shared by the launches of a run, which are ordered by the stream.
struct ddrl_update_group {
  std::vector<ddrl_ctx*> members;
  int device = 0;
  hipStream_t stream = nullptr;
  MemberTable<UpdateArgs> table;       // one entry per chain
  int P = 0, cap = 0;                  // policies per member, chains per launch
  std::vector<int32_t> launch_of_member, first_block;
  std::vector<int> launch_g0, launch_n, launch_x0;   // first chain, chains and first xcc slot of each launch
  int xcc_total = 0;
  unsigned long long *xchg = nullptr, *gx = nullptr;
  int *err = nullptr, *xcc = nullptr;
  std::vector<int> xcc_host;           // the record of the last finished run
  unsigned epoch = 0;                  // launches so far (granule tag epochs), the group's own
  int inflight = 0;                    // a run is enqueued and not yet finished
  int refused = 0;                     // a placement check failed: no further runs
};

namespace {
int group_plan(int M, int P, int max_chains, int32_t* launch_of_member, int32_t* first_block) {
  if (M < 1) return fail("update group: at least one member is needed");
  if (P < 1 || P > DDRL_MAXP) return fail("update group: n_policies must be 1 .. " + std::to_string(DDRL_MAXP));
  if (max_chains < P)
    return fail("update group: a launch of at most " + std::to_string(max_chains) + " chains cannot hold a member's " +
                std::to_string(P) + " (members are never split across launches)");
  const int per = max_chains / P;   // whole members per launch
  for (int m = 0; m < M; ++m) {
    if (launch_of_member) launch_of_member[m] = m / per;
    for (int p = 0; p < P && first_block; ++p) {
      const int lc = (m % per) * P + p;   // chain index inside its launch
      first_block[m * P + p] = 32 * (lc >> 3) + (lc & 7);
    }
  }
  return 0;
}

std::string member_name(int m) { return group_member_name("update", m); }

// what a member must still be at every run (create checks it too): the group's stream, the default
// exchange protocol, no peer
int group_member_ok(const ddrl_update_group* g, int m) {
  const ddrl_ctx* c = g->members[m];
  if (c->stream != g->stream) return fail(member_name(m) + " is on another stream than member 0");
  if (c->xchg_atomic)
    return fail(member_name(m) + " is on the atomic exchange protocol (DDRL_XCHG=atomic, or switched after a failed "
                "placement check); the group kernel has the default protocol only");
  if (c->peer_gx || c->peer_rank >= 0) return fail(member_name(m) + " is attached to a peer (ddrl_peer_attach)");
  return 0;
}

// the first difference between member m's configuration and member 0's in anything the update reads
int group_same_shape(const ddrl_ctx* a, const ddrl_ctx* b, int m) {
  const ddrl_cfg &x = a->cfg, &y = b->cfg;
  const char* why = nullptr;
  DDRL_GRP_SAME(model_kind); DDRL_GRP_SAME(n_policies); DDRL_GRP_SAME(act_dim); DDRL_GRP_SAME(leg_coupling);
  DDRL_GRP_SAME(sgd_minibatch_size); DDRL_GRP_SAME(num_sgd_iter); DDRL_GRP_SAME(clip_param);
  DDRL_GRP_SAME(vf_clip_param); DDRL_GRP_SAME(vf_loss_coeff); DDRL_GRP_SAME(entropy_coeff); DDRL_GRP_SAME(lr);
  DDRL_GRP_SAME(grad_clip); DDRL_GRP_SAME(adam_beta1); DDRL_GRP_SAME(adam_beta2); DDRL_GRP_SAME(adam_eps);
  DDRL_GRP_SAME(vf_clip_mode);
  for (int p = 0; p < x.n_policies && !why; ++p) {
    const Policy &P = a->pol[p], &Q = b->pol[p];
    if (P.d != Q.d) why = "obs_dim";
    else if (std::memcmp(&P.lay, &Q.lay, sizeof(RecLayout)) != 0) why = "the record layout";
    else if (P.R != Q.R || P.nb != Q.nb) why = "frag_len x n_envs (rows per policy)";
    else if (P.n_params != Q.n_params) why = "the parameter count";
  }
  return group_same_result("update", m, why);
}

void group_free(ddrl_update_group* g) {
  g->table.release();
  for (void* p : {(void*)g->xchg, (void*)g->gx, (void*)g->err, (void*)g->xcc})
    if (p) (void)hipFree(p);
  delete g;
}
}  // namespace

extern "C" {

int ddrl_update_group_plan(int n_members, int n_policies, int max_chains, int32_t* launch_of_member,
                           int32_t* first_block_of_chain) {
  return group_plan(n_members, n_policies, max_chains, launch_of_member, first_block_of_chain);
}

int ddrl_update_group_create(ddrl_ctx* const* members, int n_members, int max_chains_per_launch,
                             ddrl_update_group** out) {
  if (!members || !out) return fail("null argument");
  if (n_members < 1) return fail("update group: at least one member is needed");
  if (max_chains_per_launch < 0) return fail("update group: max_chains_per_launch must be >= 0 (0: the device's cap)");
  if (group_list_ok("update", members, nullptr, n_members)) return -1;
  ddrl_ctx* c0 = members[0];
  HIPCHK(hipSetDevice(c0->device));
  ddrl_update_group* g = new ddrl_update_group();
  g->members.assign(members, members + n_members);
  g->device = c0->device;
  g->stream = c0->stream;
  g->P = c0->cfg.n_policies;
  int rc = 0;
  for (int m = 0; m < n_members && !rc; ++m) {
    const ddrl_ctx* c = members[m];
    if (group_member_kind("update", c, g->device, m)) rc = -1;
    else if (c->cfg.sgd_minibatch_size != 128) rc = fail(member_name(m) + " has sgd_minibatch_size " + std::to_string(c->cfg.sgd_minibatch_size) + ": the group kernel is built for 128-row minibatches only");
    else if (c->update_split != 2) rc = fail(member_name(m) + " was created under DDRL_UPDATE_SPLIT=1: the group kernel is the row split");
    else rc = group_member_ok(g, m) || group_same_shape(c, c0, m);
  }
  int cus = 0;
  if (!rc && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->device) != hipSuccess)
    rc = fail("update group: cannot read the device's CU count");
  if (!rc) {
    // one workgroup per CU (by LDS), four per chain, a chain's four on one XCD: with the CUs in 8
    // XCDs, floor((CUs / 8) / 4) chains per XCD are resident together
    g->cap = 8 * ((cus / 8) / 4);
    if (max_chains_per_launch > 0) g->cap = std::min(g->cap, max_chains_per_launch);
    g->launch_of_member.resize(n_members);
    g->first_block.resize((size_t)n_members * g->P);
    rc = group_plan(n_members, g->P, g->cap, g->launch_of_member.data(), g->first_block.data());
  }
  if (!rc) {
    const int nl = g->launch_of_member.back() + 1;
    g->launch_g0.assign(nl, 0); g->launch_n.assign(nl, 0); g->launch_x0.assign(nl, 0);
    for (int m = 0; m < n_members; ++m) g->launch_n[g->launch_of_member[m]] += g->P;
    int maxn = 0;
    for (int l = 0; l < nl; ++l) {
      g->launch_g0[l] = l ? g->launch_g0[l - 1] + g->launch_n[l - 1] : 0;
      g->launch_x0[l] = g->xcc_total;
      g->xcc_total += update_group_grid(g->launch_n[l]);
      maxn = std::max(maxn, g->launch_n[l]);
    }
    const size_t nchain = (size_t)n_members * g->P, rows8 = 8 * (size_t)((maxn + 7) / 8);
    auto dev = [&](void** p, size_t bytes) {
      return hipMalloc(p, bytes) == hipSuccess && hipMemset(*p, 0, bytes) == hipSuccess;
    };
    if (!g->table.alloc(nchain) || !dev((void**)&g->xchg, sizeof(unsigned long long) * 8 * rows8) || !dev((void**)&g->gx, gx_bytes(maxn)) ||
        !dev((void**)&g->err, sizeof(int)) || !dev((void**)&g->xcc, sizeof(int) * (size_t)g->xcc_total) ||
        hipDeviceSynchronize() != hipSuccess)
      rc = fail("update group: allocation failed (" + std::to_string(gx_bytes(maxn) >> 20) + " MB of outboxes)");
    g->xcc_host.assign(g->xcc_total, -1);
  }
  if (rc) {
    group_free(g);
    return -1;
  }
  *out = g;
  return 0;
}

int ddrl_update_group_run(ddrl_update_group* g, const int32_t* const* shuffle, const int32_t* const* perm,
                          const float* kl, int max_steps) {
  if (!g) return fail("null update group");
  if (!shuffle || !perm || !kl) return fail("null update argument");
  if (g->refused)
    return fail("update group: an earlier run failed the placement check (a chain's workgroups ran on different "
                "XCDs), and the group kernel has no protocol for that: update the members one by one "
                "(ddrl_ppo_update, which switches to the atomic exchange)");
  if (g->inflight) return fail("update group: the previous run has not been finished (ddrl_update_group_finish)");
  const int M = (int)g->members.size(), P = g->P;
  ddrl_ctx* c0 = g->members[0];
  for (int m = 0; m < M; ++m) {
    if (group_member_ok(g, m)) return -1;
    for (int p = 0; p < P; ++p) {
      if (!shuffle[m * P + p] || !perm[m * P + p])
        return fail(member_name(m) + ": null shuffle/perm for policy " + std::to_string(p));
      if (g->members[m]->pol[p].R < 128)
        return fail(member_name(m) + ", policy " + std::to_string(p) + ": the train batch holds " +
                    std::to_string(g->members[m]->pol[p].R) + " rows, fewer than one minibatch");
    }
  }
  HIPCHK(hipSetDevice(g->device));
  UpdateArgs* table = nullptr;
  if (g->table.host(table)) return -1;
  int maxd = 0, maxs = 0, hook = 0;
  for (int m = 0; m < M; ++m) {
    ddrl_ctx* c = g->members[m];
    hook |= c->fail_step >= 0;
    for (int p = 0; p < P; ++p) {
      UpdateArgs& u = table[m * P + p];
      u = make_update(c, p, shuffle[m * P + p], perm[m * P + p], kl[m * P + p]);
      u.max_steps = max_steps;
      c->kl_last[p] = kl[m * P + p];
      const int total = c->cfg.num_sgd_iter * c->pol[p].nb;
      c->pol[p].last_steps = max_steps >= 0 ? std::min(total, max_steps) : total;
      maxd = std::max(maxd, u.d), maxs = std::max(maxs, u.lay.stride);
    }
    if (snapshot(c, (1 << P) - 1)) return -1;
  }
  if (g->table.upload(g->stream, (size_t)M * P)) return -1;
  // test hook (DDRL_TEST_FAIL_STEP on any member): the run starts with the group's error word set,
  // as launch_ffn does for a context -- every chain runs its steps and none writes back
  if (hook) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)g->err, 1, 1, g->stream));
  const UpdateHyper h = make_hyper(c0, P);
  for (size_t l = 0; l < g->launch_n.size(); ++l)
    if (launch_update_ffn_group(g->stream, g->table.dev + g->launch_g0[l], g->launch_n[l], h, c0->cfg.act_dim, maxd, maxs,
                                c0->cfg.leg_coupling, g->xchg, g->gx, g->err, &g->epoch, g->xcc + g->launch_x0[l])) {
      for (ddrl_ctx* c : g->members) c->snap_mask = 0;   // nothing ran: nothing to restore
      (void)hipMemsetAsync(g->err, 0, sizeof(int), g->stream);
      return fail("update group: this library was built without the group kernel (a diagnostic build); nothing ran");
    }
  g->inflight = 1;
  HIPCHK(hipGetLastError());
  return 0;
}

int ddrl_update_group_finish(ddrl_update_group* g) {
  if (!g) return fail("null update group");
  if (!g->inflight) return 0;
  HIPCHK(hipSetDevice(g->device));
  HIPCHK(hipStreamSynchronize(g->stream));
  g->inflight = 0;
  g->table.stream_synced();
  HIPCHK(hipGetLastError());
  int e = 0;
  HIPCHK(hipMemcpy(&e, g->err, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(g->xcc_host.data(), g->xcc, sizeof(int) * g->xcc_host.size(), hipMemcpyDeviceToHost));
  int bad = 0;
  for (size_t l = 0; l < g->launch_n.size(); ++l)
    for (int lc = 0; lc < g->launch_n[l]; ++lc) {
      const int* x = g->xcc_host.data() + g->launch_x0[l] + 32 * (lc >> 3) + (lc & 7);
      for (int j = 1; j < 4; ++j) bad |= x[8 * j] != x[0];
    }
  if (bad) g->refused = 1;
  const int full = (1 << g->P) - 1;
  if (e) {
    (void)hipMemset(g->err, 0, sizeof(int));
    // the snapshots run() took, whatever a member's own calls did to its mask since
    for (ddrl_ctx* c : g->members) {
      c->snap_mask = full;
      const int rc = restore_snapshot(c);
      c->snap_mask = 0;
      if (rc) return -1;
    }
    if (bad)
      return fail("update group: the workgroups of a chain ran on different XCDs (placement check), so the exchange "
                  "through the XCD's L2 could not complete.  The weights, Adam state and beta powers of every member "
                  "are as before the call; this group refuses further runs: update the members one by one");
    return fail("update group: an exchange between the workgroups of a chain was abandoned (3 s timeout, a grid that "
                "was not resident, or a failed launch).  The weights, Adam state and beta powers of every member are "
                "as before the call");
  }
  // a stale snapshot must never be restored by a member's later, unrelated check
  for (ddrl_ctx* c : g->members) c->snap_mask = 0;
  return 0;
}

int ddrl_update_group_placement(ddrl_update_group* g, int32_t* xcc, int n_blocks) {
  if (!g) return fail("null update group");
  if (!xcc) return fail("null placement buffer");
  if (g->inflight) return fail("update group: finish the run before reading its placement");
  if (n_blocks < g->xcc_total)
    return fail("update group: the placement record holds " + std::to_string(g->xcc_total) +
                " blocks (the launches' grids, in launch order)");
  for (int i = 0; i < n_blocks; ++i) xcc[i] = i < g->xcc_total ? g->xcc_host[i] : -1;
  return 0;
}

int ddrl_update_group_destroy(ddrl_update_group* g) {
  if (!g) return 0;
  (void)hipSetDevice(g->device);
  (void)hipStreamSynchronize(g->stream);
  group_free(g);   // (the members may be gone already: they are not touched)
  return 0;
}

}  // extern "C"

// ---- group rollout (rollout_group.hip): the device-plane fragments of M same-shaped contexts as one chain ----
// Member m is the context members[m] with its own device env plane envs[m].  The kernels read what
// differs between members from a device table of RolloutMember, rebuilt at every run from the
// members' current state (so terrain, time limit and target velocities set between runs hold) in
// the group's MemberTable.
struct ddrl_rollout_group {
  std::vector<ddrl_ctx*> members;
  std::vector<ddrl_devenv*> envs;
  int device = 0;
  hipStream_t stream = nullptr;
  MemberTable<RolloutMember> table;
};

namespace {
std::string rmember_name(int m) { return group_member_name("rollout", m); }

// the reward tables without what is per member (the record pointers)
RewardArgs shape_reward(ddrl_ctx* c) {
  RewardArgs r = make_reward(c);
  for (int p = 0; p < DDRL_MAXP; ++p) r.rec[p] = nullptr;
  return r;
}

// the first difference between member m's configuration and member 0's in anything the rollout kernels read
int rgroup_same_shape(ddrl_ctx* a, ddrl_ctx* b, int m) {
  const ddrl_cfg &x = a->cfg, &y = b->cfg;
  const char* why = nullptr;
  DDRL_GRP_SAME(model_kind); DDRL_GRP_SAME(n_envs); DDRL_GRP_SAME(frag_len); DDRL_GRP_SAME(n_policies);
  DDRL_GRP_SAME(n_agents); DDRL_GRP_SAME(act_dim); DDRL_GRP_SAME(obs_full_dim); DDRL_GRP_SAME(leg_coupling);
  DDRL_GRP_SAME(policy_filter); DDRL_GRP_SAME(filter_enabled); DDRL_GRP_SAME(filter_update);
  DDRL_GRP_SAME(filter_clip); DDRL_GRP_SAME(reward_mode); DDRL_GRP_SAME(ctrl_cost_weight);
  DDRL_GRP_SAME(contact_cost_weight);
  for (int p = 0; p < x.n_policies && !why; ++p) {
    const Policy &P = a->pol[p], &Q = b->pol[p];
    if (P.d != Q.d) why = "obs_dim";
    else if (P.k != Q.k) why = "agent_policy (agents per policy)";
    else if (std::memcmp(&P.lay, &Q.lay, sizeof(RecLayout)) != 0) why = "the record layout";
  }
  if (!why && std::memcmp(&a->route, &b->route, sizeof(RouteArgs)) != 0)
    why = "the routing tables (agent_policy, obs_index, act_index, act_negate, leg angles)";
  if (!why) {
    const RewardArgs ra = shape_reward(a), rb = shape_reward(b);
    if (std::memcmp(&ra, &rb, sizeof(RewardArgs)) != 0) why = "the reward tables (n_contact, contact_index, contact_weight)";
  }
  return group_same_result("rollout", m, why);
}
#undef DDRL_GRP_SAME

// what a member and its env must still be at every run (create checks it too)
int rgroup_member_ok(const ddrl_rollout_group* g, int m) {
  const ddrl_ctx* c = g->members[m];
  const ddrl_devenv *e = g->envs[m], *e0 = g->envs[0];
  if (!e->ctx) return fail(rmember_name(m) + ": its device env's context has been destroyed");
  if (e->ctx != c) return fail(rmember_name(m) + ": its device env is bound to another context");
  if (c->stream != g->stream) return fail(rmember_name(m) + " is on another stream than member 0");
  if (e->a.ter_on != e0->a.ter_on)
    return fail(rmember_name(m) + " has its terrain " + (e->a.ter_on ? "on" : "off") + " and member 0 " +
                (e0->a.ter_on ? "on" : "off") + ": the step kernel's instance is one per launch");
  if (!e->a.tv_env != !e0->a.tv_env)
    return fail(rmember_name(m) + " and member 0 differ in the target-velocity mode (a per-env table against draws from "
                "the list): the step kernel's instance is one per launch");
  return 0;
}

void rgroup_free(ddrl_rollout_group* g) {
  g->table.release();
  delete g;
}
}  // namespace

extern "C" {

int ddrl_rollout_group_create(ddrl_ctx* const* members, ddrl_devenv* const* envs, int n_members,
                              ddrl_rollout_group** out) {
  if (!members || !envs || !out) return fail("null argument");
  if (n_members < 1) return fail("rollout group: at least one member is needed");
  if (n_members > 65535)
    return fail("rollout group: " + std::to_string(n_members) + " members exceed the grid's z extent (65535)");
  if (group_list_ok("rollout", members, envs, n_members)) return -1;
  ddrl_ctx* c0 = members[0];
  HIPCHK(hipSetDevice(c0->device));
  ddrl_rollout_group* g = new ddrl_rollout_group();
  g->members.assign(members, members + n_members);
  g->envs.assign(envs, envs + n_members);
  g->device = c0->device;
  g->stream = c0->stream;
  int rc = 0;
  for (int m = 0; m < n_members && !rc; ++m)
    rc = group_member_kind("rollout", members[m], g->device, m) || rgroup_same_shape(members[m], c0, m);
  for (int m = 0; m < n_members && !rc; ++m) rc = rgroup_member_ok(g, m);
  if (!rc && (!g->table.alloc(n_members) || hipDeviceSynchronize() != hipSuccess))
    rc = fail("rollout group: allocation of the member table failed");
  if (rc) {
    rgroup_free(g);
    return -1;
  }
  *out = g;
  return 0;
}

int ddrl_rollout_group_run(ddrl_rollout_group* g, const float* const* eps_dev, int reset) {
  if (!g) return fail("null rollout group");
  if (!eps_dev) return fail("null noise buffer");
  const int M = (int)g->members.size();
  for (int m = 0; m < M; ++m) {
    if (!eps_dev[m]) return fail(rmember_name(m) + ": null noise buffer");
    if (rgroup_member_ok(g, m)) return -1;
  }
  HIPCHK(hipSetDevice(g->device));
  ddrl_ctx* c0 = g->members[0];
  const ddrl_cfg& cfg = c0->cfg;
  if (reset)
    for (int m = 0; m < M; ++m)
      if (ddrl_devenv_reset(g->envs[m]) || ddrl_observe(g->members[m], g->envs[m]->a.obs)) return -1;
  RolloutMember* table = nullptr;
  if (g->table.host(table)) return -1;
  for (int m = 0; m < M; ++m) {
    ddrl_ctx* c = g->members[m];
    RolloutMember& r = table[m];
    r = RolloutMember{};
    for (int p = 0; p < cfg.n_policies; ++p) {
      Policy& P = c->pol[p];
      r.theta[p] = P.theta; r.stage[p] = P.stage; r.rec[p] = P.rec; r.last_v[p] = P.last_v;
      r.cup[p] = cup_table(c, p);
    }
    r.eps = eps_dev[m]; r.actions = c->h_act; r.done_tn = c->done_tn;
    r.f_n = c->f_n; r.f_M = c->f_M; r.f_S = c->f_S; r.f_normc = c->f_normc;
    r.f_dn = c->f_dn; r.f_dM = c->f_dM; r.f_dS = c->f_dS; r.f_part = c->f_part;
    r.pf = cfg.policy_filter ? c->pf : nullptr;
    r.zs = c->zs;
    r.env = g->envs[m]->a;
  }
  if (g->table.upload(g->stream, M)) return -1;
  RolloutGroupArgs ga{};
  ga.tab = g->table.dev; ga.M = M; ga.n = cfg.n_envs; ga.T = cfg.frag_len;
  for (int p = 0; p < cfg.n_policies; ++p) {
    ga.lay[p] = c0->pol[p].lay;
    ga.C[p] = c0->pol[p].C;
  }
  ga.filter_update = cfg.filter_update; ga.filter_enabled = cfg.filter_enabled; ga.policy_filter = cfg.policy_filter;
  ga.clip = effective_clip(cfg);
  ga.ter_on = g->envs[0]->a.ter_on; ga.tv_env = g->envs[0]->a.tv_env ? 1 : 0;
  const RewardArgs rw = shape_reward(c0);
  // issued directly: the same chain as one replayed HIP graph was no faster (DESIGN.md section 3,
  // "Population rollout"; profiles/population/rollout_graph_ab.json)
  for (int t = 0; t < cfg.frag_len; ++t) launch_rollout_group_step(g->stream, c0->route, rw, ga, t);
  launch_rollout_group_bootstrap(g->stream, c0->route, ga);
  HIPCHK(hipGetLastError());
  // what the plain calls would have noted on every member
  for (ddrl_ctx* c : g->members) {
    c->ep_collected = 0;
    c->ev_normc_ok = 0;
    c->sens_act_ok = 0;
  }
  return 0;
}

int ddrl_rollout_group_destroy(ddrl_rollout_group* g) {
  if (!g) return 0;
  (void)hipSetDevice(g->device);
  (void)hipStreamSynchronize(g->stream);
  rgroup_free(g);   // (the members may be gone already: they are not touched)
  return 0;
}

}  // extern "C"

// ---- device randomness (rng.hip): noise and schedules drawn on the device ----
// A stream is (seed, position) on the host; every launch gets both by value (solo) or through a
// member table (group), so the calls are asynchronous and a captured graph never holds a position.
struct RngTables {
  MemberTable<NoiseMember> noise;
  MemberTable<ScheduleMember> sched;
  int noise_cap = 0, sched_cap = 0;
};

static void rng_tables_free(RngTables* t) {
  if (t->noise_cap) t->noise.release();
  if (t->sched_cap) t->sched.release();
  delete t;
}

namespace {
const char* const kRngName[2] = {"noise", "schedule"};

int rng_stream_ok(int stream) {
  if (stream != DDRL_RNG_NOISE && stream != DDRL_RNG_SCHEDULE) return fail("rng: stream must be DDRL_RNG_NOISE or DDRL_RNG_SCHEDULE");
  return 0;
}

std::string rng_unseeded(int stream) {
  return std::string("the ") + kRngName[stream] + " stream has no seed: call ddrl_rng_seed or ddrl_rng_state_set first";
}

// Philox blocks per env, or a refusal
int noise_blocks(const ddrl_ctx* c, int* B) {
  const int comps = c->cfg.n_agents * c->cfg.act_dim;
  if (comps < 4 || comps % 4)
    return fail("noise fill: n_agents * act_dim = " + std::to_string(comps) + " is not a multiple of 4 (one Philox block is four normals)");
  *B = comps / 4;
  return 0;
}

int noise_args_ok(int n_steps, const float* eps, const std::string& who) {
  if (n_steps < 1) return fail("noise fill: n_steps must be >= 1");
  if (!eps) return fail(who + "null noise buffer");
  if ((uintptr_t)eps % 16) return fail(who + "the noise buffer is not 16-byte aligned");
  return 0;
}

ScheduleShape schedule_shape(const ddrl_ctx* c, int mask) {
  ScheduleShape sh{};
  for (int p = 0; p < c->cfg.n_policies; ++p) {
    sh.R[p] = c->pol[p].R;
    sh.nb[p] = c->pol[p].nb;
    if (mask & (1 << p)) sh.pid[sh.n_pol++] = p;
  }
  sh.epochs = c->cfg.num_sgd_iter;
  return sh;
}

// the table of a group fill with room for n members: member 0's, grown behind a stream synchronize
template <class T>
int rng_table(ddrl_ctx* c0, MemberTable<T> RngTables::*tab, int RngTables::*cap, int n, MemberTable<T>** out) {
  if (!c0->rng_tabs) c0->rng_tabs = new RngTables();
  RngTables* t = c0->rng_tabs;
  if (t->*cap < n) {
    if (t->*cap) {
      HIPCHK(hipStreamSynchronize(c0->stream));   // the last fill read the old table
      (t->*tab).release();
      t->*tab = MemberTable<T>{};
      t->*cap = 0;
    }
    if (!(t->*tab).alloc(n)) {
      (t->*tab).release();
      t->*tab = MemberTable<T>{};
      return fail("group fill: allocation of the member table failed");
    }
    t->*cap = n;
  }
  *out = &(t->*tab);
  return 0;
}

// what both group fills ask of their member list; `kind` is "noise fill" or "schedule fill"
int rng_group_ok(const char* kind, ddrl_ctx* const* members, int n_members, int stream) {
  if (!members) return fail("null argument");
  if (n_members < 1) return fail(std::string(kind) + " group: at least one member is needed");
  if (n_members > 65535)
    return fail(std::string(kind) + " group: " + std::to_string(n_members) + " members exceed the grid's z extent (65535)");
  if (group_list_ok(kind, members, nullptr, n_members)) return -1;
  const ddrl_ctx* c0 = members[0];
  for (int m = 0; m < n_members; ++m) {
    const ddrl_ctx* c = members[m];
    if (c->device != c0->device) return fail(group_member_name(kind, m) + " is on another device than member 0");
    if (c->stream != c0->stream) return fail(group_member_name(kind, m) + " is on another stream than member 0");
    if (!c->rng[stream].seeded) return fail(group_member_name(kind, m) + ": " + rng_unseeded(stream));
  }
  return 0;
}
}  // namespace

extern "C" {

int ddrl_rng_seed(ddrl_ctx* c, int stream, uint64_t seed) { return ddrl_rng_state_set(c, stream, seed, 0); }

int ddrl_rng_state_set(ddrl_ctx* c, int stream, uint64_t seed, uint64_t position) {
  CHK_CTX(c);
  if (rng_stream_ok(stream)) return -1;
  c->rng[stream].seed = seed;
  c->rng[stream].pos = position;
  c->rng[stream].seeded = 1;
  return 0;
}

int ddrl_rng_state_get(ddrl_ctx* c, int stream, uint64_t* seed, uint64_t* position) {
  CHK_CTX(c);
  if (rng_stream_ok(stream)) return -1;
  if (!seed || !position) return fail("null argument");
  if (!c->rng[stream].seeded) return fail(rng_unseeded(stream));
  *seed = c->rng[stream].seed;
  *position = c->rng[stream].pos;
  return 0;
}

int ddrl_noise_fill(ddrl_ctx* c, int n_steps, float* eps_dev) {
  CHK_CTX(c);
  ddrl_ctx::RngStream& st = c->rng[DDRL_RNG_NOISE];
  int B = 0;
  if (!st.seeded) return fail(rng_unseeded(DDRL_RNG_NOISE));
  if (noise_args_ok(n_steps, eps_dev, "noise fill: ") || noise_blocks(c, &B)) return -1;
  HIPCHK(hipSetDevice(c->device));
  launch_noise_fill(c->stream, NoiseMember{eps_dev, st.seed, st.pos}, n_steps, c->cfg.n_envs, B);
  HIPCHK(hipGetLastError());
  st.pos += (uint64_t)n_steps;
  return 0;
}

int ddrl_schedule_fill(ddrl_ctx* c, int pid_mask, int32_t* const* shuffle_dev, int32_t* const* perm_dev) {
  CHK_CTX(c);
  ddrl_ctx::RngStream& st = c->rng[DDRL_RNG_SCHEDULE];
  if (!st.seeded) return fail(rng_unseeded(DDRL_RNG_SCHEDULE));
  if (!shuffle_dev || !perm_dev) return fail("schedule fill: null schedule table");
  if (pid_mask <= 0 || (pid_mask >> c->cfg.n_policies))
    return fail("schedule fill: pid_mask " + std::to_string(pid_mask) + " names no policy or one outside the context's " +
                std::to_string(c->cfg.n_policies));
  ScheduleMember sm{};
  for (int p = 0; p < c->cfg.n_policies; ++p) {
    if (!(pid_mask & (1 << p))) continue;
    if (!shuffle_dev[p] || !perm_dev[p]) return fail("schedule fill: null schedule buffer of policy " + std::to_string(p));
    sm.shuffle[p] = shuffle_dev[p];
    sm.perm[p] = perm_dev[p];
  }
  sm.seed = st.seed;
  sm.draw = st.pos;
  HIPCHK(hipSetDevice(c->device));
  launch_schedule_fill(c->stream, sm, schedule_shape(c, pid_mask));
  HIPCHK(hipGetLastError());
  st.pos += 1;
  return 0;
}

int ddrl_noise_fill_group(ddrl_ctx* const* members, int n_members, int n_steps, float* const* eps_dev) {
  const char* kind = "noise fill";
  if (rng_group_ok(kind, members, n_members, DDRL_RNG_NOISE)) return -1;
  if (!eps_dev) return fail("noise fill group: null noise buffer");
  ddrl_ctx* c0 = members[0];
  int B = 0;
  if (noise_blocks(c0, &B)) return -1;
  for (int m = 0; m < n_members; ++m) {
    const ddrl_cfg &x = members[m]->cfg, &y = c0->cfg;
    const char* why = x.n_envs != y.n_envs ? "n_envs" : x.n_agents != y.n_agents ? "n_agents" : x.act_dim != y.act_dim ? "act_dim" : nullptr;
    if (group_same_result(kind, m, why) || noise_args_ok(n_steps, eps_dev[m], group_member_name(kind, m) + ": ")) return -1;
  }
  HIPCHK(hipSetDevice(c0->device));
  MemberTable<NoiseMember>* tab = nullptr;
  NoiseMember* host = nullptr;
  if (rng_table(c0, &RngTables::noise, &RngTables::noise_cap, n_members, &tab) || tab->host(host)) return -1;
  for (int m = 0; m < n_members; ++m) {
    const ddrl_ctx::RngStream& st = members[m]->rng[DDRL_RNG_NOISE];
    host[m] = NoiseMember{eps_dev[m], st.seed, st.pos};
  }
  if (tab->upload(c0->stream, n_members)) return -1;
  launch_noise_fill_group(c0->stream, tab->dev, n_members, n_steps, c0->cfg.n_envs, B);
  HIPCHK(hipGetLastError());
  for (int m = 0; m < n_members; ++m) members[m]->rng[DDRL_RNG_NOISE].pos += (uint64_t)n_steps;
  return 0;
}

int ddrl_schedule_fill_group(ddrl_ctx* const* members, int n_members, int32_t* const* shuffle_dev,
                             int32_t* const* perm_dev) {
  const char* kind = "schedule fill";
  if (rng_group_ok(kind, members, n_members, DDRL_RNG_SCHEDULE)) return -1;
  if (!shuffle_dev || !perm_dev) return fail("schedule fill group: null schedule table");
  ddrl_ctx* c0 = members[0];
  const int P = c0->cfg.n_policies;
  for (int m = 0; m < n_members; ++m) {
    const ddrl_ctx* c = members[m];
    const char* why = c->cfg.n_policies != P ? "n_policies" : c->cfg.num_sgd_iter != c0->cfg.num_sgd_iter ? "num_sgd_iter" : nullptr;
    for (int p = 0; p < P && !why; ++p)
      if (c->pol[p].R != c0->pol[p].R || c->pol[p].nb != c0->pol[p].nb) why = "the rows or minibatches of a policy";
    if (group_same_result(kind, m, why)) return -1;
    for (int p = 0; p < P; ++p)
      if (!shuffle_dev[m * P + p] || !perm_dev[m * P + p])
        return fail(group_member_name(kind, m) + ": null schedule buffer of policy " + std::to_string(p));
  }
  HIPCHK(hipSetDevice(c0->device));
  MemberTable<ScheduleMember>* tab = nullptr;
  ScheduleMember* host = nullptr;
  if (rng_table(c0, &RngTables::sched, &RngTables::sched_cap, n_members, &tab) || tab->host(host)) return -1;
  for (int m = 0; m < n_members; ++m) {
    const ddrl_ctx::RngStream& st = members[m]->rng[DDRL_RNG_SCHEDULE];
    ScheduleMember sm{};
    for (int p = 0; p < P; ++p) {
      sm.shuffle[p] = shuffle_dev[m * P + p];
      sm.perm[p] = perm_dev[m * P + p];
    }
    sm.seed = st.seed;
    sm.draw = st.pos;
    host[m] = sm;
  }
  if (tab->upload(c0->stream, n_members)) return -1;
  launch_schedule_fill_group(c0->stream, tab->dev, n_members, schedule_shape(c0, (1 << P) - 1));
  HIPCHK(hipGetLastError());
  for (int m = 0; m < n_members; ++m) members[m]->rng[DDRL_RNG_SCHEDULE].pos += 1;
  return 0;
}

}  // extern "C"
