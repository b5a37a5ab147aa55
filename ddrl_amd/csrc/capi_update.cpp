// C-ABI of libddrl_hip.so: GAE and the PPO update (fused, gradient / apply, data-parallel, peer), the forward pass.
#include "ctx.h"

namespace ddrl_impl {
UpdateHyper make_hyper(ddrl_ctx* c, int P) {
  const ddrl_cfg& g = c->cfg;
  UpdateHyper h{};
  h.clip = g.clip_param; h.vf_clip = g.vf_clip_param; h.vf_coeff = g.vf_loss_coeff;
  h.ent_coeff = g.entropy_coeff; h.lr = g.lr; h.grad_clip = g.grad_clip; h.b1 = g.adam_beta1;
  h.b2 = g.adam_beta2; h.eps = g.adam_eps; h.vf_mode = g.vf_clip_mode; h.P = P;
  return h;
}

UpdateArgs make_update(ddrl_ctx* c, int p, const int32_t* shuffle, const int32_t* perm, float kl) {
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
}  // namespace ddrl_impl

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

extern "C" {

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
    c->pol[p].last_steps = steps_to_run(total, step0, max_steps);
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
  CHK_PID(c, pid);
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

// the one-step gradient form of policy pid's update over `rows` (one minibatch slice, or a rank's share of one):
// no Adam step, the gradient goes to grad_out; the caller sets the statistics row
static UpdateArgs make_grad_step(ddrl_ctx* c, int pid, const int32_t* rows, float kl, float* grad_out) {
  UpdateArgs u = make_update(c, pid, rows, c->zero_perm, kl);
  u.nb = 1; u.n_epochs = 1; u.max_steps = 1; u.step0 = 0; u.grad_out = grad_out;
  return u;
}

int ddrl_ppo_grad(ddrl_ctx* c, int pid, const int32_t* rows, int n_rows, float kl, float* grad,
                  int stats_step) {
  CHK_CTX(c);
  CHK_PID(c, pid);
  if (n_rows < 1 || n_rows > 128) return fail("n_rows must be in [1, 128]");
  if (!rows || !grad) return fail("null rows/grad");
  if (stats_step >= 0 && (size_t)stats_step >= c->pol[pid].stats_steps &&
      stats_reserve(c, pid, std::max((size_t)stats_step + 1, 2 * c->pol[pid].stats_steps)))
    return -1;
  UpdateArgs u = make_grad_step(c, pid, rows, kl, grad);
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
  CHK_PID(c, pid);
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
  CHK_PID(c, pid);
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
      UpdateArgs u = make_grad_step(c, pid, shuffle + (size_t)slot * m, kl, P.grad);
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
  if (dgrow(c, &c->ddp_chunk, &c->ddp_chunk_n, need) || dgrow(c, &c->ddp_slots, &c->ddp_slots_n, (size_t)steps)) return -1;
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
    if (dgrow(c, &P.stats, &P.stats_steps, E * nb, 8)) return -1;
  }
  if (c->peer_vsh_n < nb * DDRL_MB) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (dgrow(c, &c->peer_vsh, &c->peer_vsh_n, nb * DDRL_MB)) return -1;
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
  CHK_PID(c, pid);
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
  P.last_steps = steps_to_run(E * nb, 0, max_steps);
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
  CHK_PID(c, pid);
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

}  // extern "C"
