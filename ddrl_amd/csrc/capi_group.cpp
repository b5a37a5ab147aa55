// C-ABI of libddrl_hip.so: the groups of contexts (update, rollout, finish) and the checks every group shares.
#include "ctx.h"

// ---- what the groups of contexts (update, rollout, finish) share; `kind` is "update", "rollout" or "finish" ----
namespace ddrl_impl {
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

int group_same_result(const char* kind, int m, const char* why) {
  return why ? fail(group_member_name(kind, m) + " differs from member 0 in " + why + ": a group takes contexts of one shape") : 0;
}
}  // namespace ddrl_impl

namespace {
// create: member m is an fcnet context on the group's device
int group_member_kind(const char* kind, const ddrl_ctx* c, int device, int m) {
  if (c->device != device) return fail(group_member_name(kind, m) + " is on another device than member 0");
  if (c->cfg.model_kind != DDRL_MODEL_FFN)
    return fail(group_member_name(kind, m) + " is a GraphNet context: the group " + kind + " runs the fcnet kernels only");
  return 0;
}

// same-shape checks: `why` names the first difference from member 0, found field by field (x.f against y.f)
#define DDRL_GRP_SAME(f) if (!why && !(x.f == y.f)) why = #f
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
  PinnedStage stage;                   // stats_range's copies land here first
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
  g->stage.release();
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
    auto dev = [](void** p, size_t bytes) { return dev_zalloc(p, bytes) == hipSuccess; };
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
      c->pol[p].last_steps = steps_to_run(c->cfg.num_sgd_iter * c->pol[p].nb, 0, max_steps);
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

// ddrl_ppo_stats_range of every chain: the copies are enqueued together and waited for once, with every
// member's error word behind them; a set word is then handled by that member's own check.
int ddrl_update_group_stats_range(ddrl_update_group* g, size_t first, size_t n_steps, float* host) {
  if (!g) return fail("null update group");
  if (!host && n_steps) return fail("null stats buffer");
  if (g->inflight) return fail("update group: finish the run before reading its statistics (ddrl_update_group_finish)");
  const int M = (int)g->members.size(), P = g->P;
  for (int m = 0; m < M; ++m)
    for (int p = 0; p < P; ++p) {
      const size_t cap = g->members[m]->pol[p].stats_steps;
      if (first > cap || n_steps > cap - first)
        return fail(member_name(m) + ", policy " + std::to_string(p) + ": more stats requested than the schedule holds");
    }
  HIPCHK(hipSetDevice(g->device));
  // pinned staging: [M][P][n_steps][8] floats, then the members' error words
  const size_t rows_bytes = (size_t)M * P * n_steps * 8 * sizeof(float);
  if (g->stage.fit(rows_bytes + sizeof(int) * M)) return -1;
  float* rows = (float*)g->stage.p;
  int* errs = (int*)(g->stage.p + rows_bytes);
  for (int m = 0; m < M; ++m) {
    const ddrl_ctx* c = g->members[m];
    for (int p = 0; p < P && n_steps; ++p)
      HIPCHK(hipMemcpyAsync(rows + ((size_t)m * P + p) * n_steps * 8, c->pol[p].stats + first * 8, n_steps * 8 * 4,
                            hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(&errs[m], c->err, sizeof(int), hipMemcpyDeviceToHost, g->stream));
  }
  HIPCHK(hipStreamSynchronize(g->stream));
  for (int m = 0; m < M; ++m)
    if (errs[m] && check_err(g->members[m])) return -1;
  if (rows_bytes) std::memcpy(host, rows, rows_bytes);
  // total_loss, as ddrl_ppo_stats_range forms it: mean(-surr) + beta*mean(kl) + vf_coeff*mean(vf) - ent_coeff*mean(H)
  for (int m = 0; m < M; ++m) {
    const ddrl_ctx* c = g->members[m];
    for (int p = 0; p < P; ++p) {
      const float beta = c->kl_last[p];
      for (size_t k = 0; k < n_steps; ++k) {
        float* s = host + (((size_t)m * P + p) * n_steps + k) * 8;
        s[0] = s[1] + beta * s[3] + c->cfg.vf_loss_coeff * s[2] - c->cfg.entropy_coeff * s[4];
      }
    }
  }
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
  for (ddrl_ctx* c : g->members) rollout_ran(c);
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

// ---- group finish (finish_group.hip): GAE and the episode accounting of M same-shaped contexts as one chain ----
// Member m is the context members[m]: whatever holds its fragment (the synthetic, host or device env
// plane), the finish reads the records only.  The FinishMember table is rebuilt at every run from the
// members' current state, so buffers replaced between runs (the episode table's growth) hold.
struct ddrl_finish_group {
  std::vector<ddrl_ctx*> members;
  int device = 0;
  hipStream_t stream = nullptr;
  MemberTable<FinishMember> table;
  long long *totals = nullptr, *totals_host = nullptr;   // [M] device, [M] pinned
  PinnedStage stage;                                     // rows' copies land here first
};

namespace {
std::string fmember_name(int m) { return group_member_name("finish", m); }

// the first difference between member m's configuration and member 0's in anything the finish kernels read
int fgroup_same_shape(const ddrl_ctx* a, const ddrl_ctx* b, int m) {
  const ddrl_cfg &x = a->cfg, &y = b->cfg;
  const char* why = nullptr;
  DDRL_GRP_SAME(n_envs); DDRL_GRP_SAME(frag_len); DDRL_GRP_SAME(n_agents); DDRL_GRP_SAME(n_policies);
  for (int j = 0; j < x.n_agents && !why; ++j)
    if (x.agent_policy[j] != y.agent_policy[j]) why = "agent_policy";
  for (int p = 0; p < x.n_policies && !why; ++p) {
    const Policy &P = a->pol[p], &Q = b->pol[p];
    if (P.k != Q.k || std::memcmp(P.agents, Q.agents, sizeof(P.agents)) != 0) why = "agent_policy";
    else if (std::memcmp(&P.lay, &Q.lay, sizeof(RecLayout)) != 0) why = "the record layout";
  }
  DDRL_GRP_SAME(gamma); DDRL_GRP_SAME(lambda_);
  return group_same_result("finish", m, why);
}
#undef DDRL_GRP_SAME

int fgroup_member_ok(const ddrl_finish_group* g, int m) {
  if (g->members[m]->stream != g->stream) return fail(fmember_name(m) + " is on another stream than member 0");
  return 0;
}

void fgroup_free(ddrl_finish_group* g) {
  g->table.release();
  g->stage.release();
  if (g->totals) (void)hipFree(g->totals);
  if (g->totals_host) (void)hipHostFree(g->totals_host);
  delete g;
}
}  // namespace

extern "C" {

int ddrl_finish_group_create(ddrl_ctx* const* members, int n_members, ddrl_finish_group** out) {
  if (!members || !out) return fail("null argument");
  if (n_members < 1) return fail("finish group: at least one member is needed");
  if (n_members > 65535)
    return fail("finish group: " + std::to_string(n_members) + " members exceed the grid's z extent (65535)");
  if (group_list_ok("finish", members, nullptr, n_members)) return -1;
  ddrl_ctx* c0 = members[0];
  HIPCHK(hipSetDevice(c0->device));
  ddrl_finish_group* g = new ddrl_finish_group();
  g->members.assign(members, members + n_members);
  g->device = c0->device;
  g->stream = c0->stream;
  int rc = 0;
  for (int m = 0; m < n_members && !rc; ++m) {
    if (members[m]->device != g->device) rc = fail(fmember_name(m) + " is on another device than member 0");
    else rc = fgroup_member_ok(g, m) || fgroup_same_shape(members[m], c0, m);
  }
  if (!rc && (!g->table.alloc(n_members) || dev_zalloc((void**)&g->totals, sizeof(long long) * n_members) != hipSuccess ||
              hipHostMalloc((void**)&g->totals_host, sizeof(long long) * n_members, hipHostMallocDefault) != hipSuccess ||
              hipDeviceSynchronize() != hipSuccess))
    rc = fail("finish group: allocation of the member table failed");
  if (rc) {
    fgroup_free(g);
    return -1;
  }
  *out = g;
  return 0;
}

int ddrl_finish_group_run(ddrl_finish_group* g, int64_t* n_finished) {
  if (!g) return fail("null finish group");
  if (!n_finished) return fail("finish group: null count output");
  const int M = (int)g->members.size();
  // refusals first: nothing is launched, no member is left half finished
  for (int m = 0; m < M; ++m) {
    if (fgroup_member_ok(g, m)) return -1;
    if (g->members[m]->ep_collected)
      return fail(fmember_name(m) + ": this fragment has been collected (collect once per fragment, after its last "
                  "reward); nothing ran on any member");
  }
  HIPCHK(hipSetDevice(g->device));
  for (ddrl_ctx* c : g->members)
    if (ep_state(c)) return -1;
  ddrl_ctx* c0 = g->members[0];
  const ddrl_cfg& cfg = c0->cfg;
  FinishMember* table = nullptr;
  if (g->table.host(table)) return -1;
  for (int m = 0; m < M; ++m) {
    ddrl_ctx* c = g->members[m];
    FinishMember& f = table[m];
    f = FinishMember{};
    for (int p = 0; p < cfg.n_policies; ++p) {
      Policy& P = c->pol[p];
      f.rec[p] = P.rec; f.last_v[p] = P.last_v; f.partials[p] = P.partials; f.adv_norm[p] = P.adv_norm;
    }
    f.done_tn = c->done_tn;
    f.ep_cnt = c->ep_cnt; f.ep_base = c->ep_base; f.ep_word = c->ep_word;
    f.ep_total = c->ep_total; f.ep_agent = c->ep_agent; f.ep_len = c->ep_len;
    f.ep_table = c->ep_table; f.ep_cap = c->ep_cap;
  }
  if (g->table.upload(g->stream, M)) return -1;
  FinishGroupArgs fa{};
  fa.tab = g->table.dev; fa.totals = g->totals;
  fa.M = M; fa.P = cfg.n_policies; fa.T = cfg.frag_len; fa.N = cfg.n_envs; fa.W = (cfg.n_envs + 63) / 64;
  fa.n_agents = cfg.n_agents;
  fa.gamma = cfg.gamma; fa.lambda_ = cfg.lambda_;
  const RewardArgs ra = make_reward(c0);   // the agent -> policy / slot maps, as ddrl_episodes_collect takes them
  for (int p = 0; p < cfg.n_policies; ++p) {
    fa.k[p] = c0->pol[p].k; fa.C[p] = c0->pol[p].C; fa.lay[p] = c0->pol[p].lay;
  }
  for (int j = 0; j < cfg.n_agents; ++j) {
    fa.policy_of_agent[j] = ra.policy_of_agent[j];
    fa.slot_of_agent[j] = ra.slot_of_agent[j];
  }
  launch_finish_group_gae(g->stream, fa);
  launch_finish_group_count_scan(g->stream, fa);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(g->totals_host, g->totals, sizeof(long long) * M, hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipStreamSynchronize(g->stream));   // the one synchronize of the group: nothing in flight reads a table either
  g->table.stream_synced();
  for (int m = 0; m < M; ++m) {
    ddrl_ctx* c = g->members[m];
    if (ep_table_fit(c, g->totals_host[m])) return -1;
    table[m].ep_table = c->ep_table;
    table[m].ep_cap = c->ep_cap;
  }
  if (g->table.upload(g->stream, M)) return -1;
  launch_finish_group_walk(g->stream, fa);
  HIPCHK(hipGetLastError());
  for (int m = 0; m < M; ++m) {
    ddrl_ctx* c = g->members[m];
    c->ep_collected = 1;
    c->ep_rows = g->totals_host[m];
    n_finished[m] = (int64_t)g->totals_host[m];
  }
  return 0;
}

int ddrl_finish_group_rows(ddrl_finish_group* g, double* const* host, const int64_t* n_rows) {
  if (!g) return fail("null finish group");
  if (!host || !n_rows) return fail("finish group: null rows argument");
  const int M = (int)g->members.size();
  for (int m = 0; m < M; ++m) {
    const ddrl_ctx* c = g->members[m];
    if (fgroup_member_ok(g, m)) return -1;
    if (c->ep_rows < 0) return fail(fmember_name(m) + ": run the group (or ddrl_episodes_collect) first");
    if (n_rows[m] != (int64_t)c->ep_rows) return fail(fmember_name(m) + ": n_rows differs from the last collect's count");
    if (n_rows[m] && !host[m]) return fail(fmember_name(m) + ": null rows buffer");
  }
  HIPCHK(hipSetDevice(g->device));
  // every member's rows into the pinned staging, one synchronize, then out to the caller's arrays
  size_t total = 0;
  for (int m = 0; m < M; ++m) total += (size_t)n_rows[m] * 8 * sizeof(double);
  if (g->stage.fit(total)) return -1;
  size_t off = 0;
  for (int m = 0; m < M; ++m) {
    const size_t bytes = (size_t)n_rows[m] * 8 * sizeof(double);
    if (bytes) HIPCHK(hipMemcpyAsync(g->stage.p + off, g->members[m]->ep_table, bytes, hipMemcpyDeviceToHost, g->stream));
    off += bytes;
  }
  HIPCHK(hipStreamSynchronize(g->stream));
  off = 0;
  for (int m = 0; m < M; ++m) {
    const size_t bytes = (size_t)n_rows[m] * 8 * sizeof(double);
    if (bytes) std::memcpy(host[m], g->stage.p + off, bytes);
    off += bytes;
  }
  return 0;
}

int ddrl_finish_group_destroy(ddrl_finish_group* g) {
  if (!g) return 0;
  (void)hipSetDevice(g->device);
  (void)hipStreamSynchronize(g->stream);
  fgroup_free(g);   // (the members may be gone already: they are not touched)
  return 0;
}

}  // extern "C"
