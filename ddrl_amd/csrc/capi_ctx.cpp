// C-ABI of libddrl_hip.so (declared in include/ddrl_hip.h): the context and its state.
// Owns every device buffer of a training shard; all work is enqueued on one HIP stream.
#include "ctx.h"

namespace {
thread_local std::string g_err;

int gnn_param_count(int A, int layer) { return gnn_param_total(A, layer); }
}  // namespace

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

namespace ddrl_impl {
int fail(const std::string& msg) {
  g_err = msg;
  return -1;
}

// Snapshot of the policies an fcnet update launch is about to change (stream-ordered D2D copies:
// theta | m | v | beta powers), restored by check_err when the launch fails.
int snapshot(ddrl_ctx* c, int mask) {
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

int restore_snapshot(ddrl_ctx* c) {
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

// A failed peer launch may have left partly written outboxes on both ranks: the pair must
// re-attach (rank 0's attach clears them) before another peer update, or a retry's tag bit could
// admit the aborted launch's stale quads.  Detaching makes ddrl_ppo_update_peer
// refuse ("no peer") until ddrl_peer_attach runs again.
void peer_detach(ddrl_ctx* c) {
  c->peer_gx = nullptr;
  c->peer_rank = -1;
  c->peer_inflight = 0;
}

int check_err(ddrl_ctx* c) {
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
}  // namespace ddrl_impl

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
  CHK_PID(c, pid);
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
  CHK_PID(c, pid);
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
  CHK_PID(c, pid);
  const Policy& P = c->pol[pid];
  const size_t nblocks = (P.C + 255) / 256;
  HIPCHK(hipMemcpyAsync(host3, P.partials + 2 * nblocks, 3 * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_records_get(ddrl_ctx* c, int pid, float* host, size_t n) {
  CHK_CTX(c);
  CHK_PID(c, pid);
  const Policy& P = c->pol[pid];
  if (n != (size_t)P.R * P.lay.stride) return fail("record buffer size mismatch");
  HIPCHK(hipMemcpyAsync(host, P.rec, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_records_set(ddrl_ctx* c, int pid, const float* host, size_t n) {
  CHK_CTX(c);
  CHK_PID(c, pid);
  const Policy& P = c->pol[pid];
  if (n != (size_t)P.R * P.lay.stride) return fail("record buffer size mismatch");
  HIPCHK(hipMemcpyAsync(P.rec, host, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->ep_collected = 0;
  return 0;
}

int ddrl_adv_norm_get(ddrl_ctx* c, int pid, float* host2) {
  CHK_CTX(c);
  CHK_PID(c, pid);
  HIPCHK(hipMemcpyAsync(host2, c->pol[pid].adv_norm, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_adv_norm_set(ddrl_ctx* c, int pid, float mean, float den) {
  CHK_CTX(c);
  CHK_PID(c, pid);
  float a[2] = {mean, den};
  HIPCHK(hipMemcpyAsync(c->pol[pid].adv_norm, a, 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_last_values_get(ddrl_ctx* c, int pid, float* host, size_t n) {
  CHK_CTX(c);
  CHK_PID(c, pid);
  if (n != (size_t)c->pol[pid].C) return fail("last value count mismatch");
  HIPCHK(hipMemcpyAsync(host, c->pol[pid].last_v, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ddrl_last_values_set(ddrl_ctx* c, int pid, const float* host, size_t n) {
  CHK_CTX(c);
  CHK_PID(c, pid);
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
  CHK_PID(c, pid);
  Policy& P = c->pol[pid];
  if (records) *records = P.rec;
  if (last_v) *last_v = P.last_v;
  if (params) *params = P.theta;
  if (adv_norm) *adv_norm = P.adv_norm;
  return 0;
}

}  // extern "C"
