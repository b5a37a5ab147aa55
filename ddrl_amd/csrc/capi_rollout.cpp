// C-ABI of libddrl_hip.so: the training rollout (observe / act / reward / bootstrap, the fragment over buffers and
// over a host env plane) and its episode accounting.
#include "ctx.h"

static int check_range(const ddrl_ctx* c, int e0, int e1) {
  if (e0 < 0 || e1 > c->cfg.n_envs || e0 >= e1) return fail("env range [e0, e1) must lie in [0, n_envs) and be non-empty");
  return 0;
}

namespace ddrl_impl {
// the reward tables of the context (record pointers included; env range and t by the caller)
RewardArgs make_reward(ddrl_ctx* c) {
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

// What `launches` issues on c->stream, run as one HIP graph: replayed from *exec, or, when there is none or the
// caller's key for it is stale, captured into a new one first (the caller then records the new key).
int graph_run(ddrl_ctx* c, hipGraphExec_t* exec, bool stale, const std::function<int()>& launches) {
  if (!*exec || stale) {
    if (*exec) {
      HIPCHK(hipGraphExecDestroy(*exec));
      *exec = nullptr;
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
    const int rc = launches();
    hipGraph_t graph = nullptr;
    e = hipStreamEndCapture(c->stream, &graph);
    c->stream = user;
    if (rc) {
      if (graph) (void)hipGraphDestroy(graph);
      return -1;
    }
    if (e != hipSuccess) return fail(std::string("rollout graph capture: ") + hipGetErrorString(e));
    const hipError_t ei = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) {
      *exec = nullptr;
      return fail(std::string("rollout graph instantiate: ") + hipGetErrorString(ei));
    }
  }
  HIPCHK(hipGraphLaunch(*exec, c->stream));
  return 0;
}

// what a rollout's observe and reward calls note on the host, for the paths that do not make those calls (a
// replayed graph, the group kernels): the fragment is new to the episode accounting, the filter constants have moved
void rollout_ran(ddrl_ctx* c) {
  c->ep_collected = 0;
  c->ev_normc_ok = 0;
  c->sens_act_ok = 0;
}
}  // namespace ddrl_impl

extern "C" {

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
  const bool stale = !std::equal(key, key + 6, c->rg_key);
  if (graph_run(c, &c->rg_exec, stale, [&] { return rollout_launches(c, obs, eps, fw, cfrc, done, actions); })) return -1;
  if (stale) std::copy(key, key + 6, c->rg_key);
  rollout_ran(c);
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

// ---- episode accounting of the training rollout (episodes.hip) ---------------------------
// Nothing here writes a record, done_tn, last_v, a filter, Adam state or a parameter.
}  // extern "C"

namespace ddrl_impl {
int ep_state(ddrl_ctx* c) {
  if (c->ep_total) return 0;
  const size_t N = c->cfg.n_envs, TW = (size_t)c->cfg.frag_len * ((N + 63) / 64);
  return dalloc(c, &c->ep_total, N) || dalloc(c, &c->ep_agent, N * DDRL_MAXAG) || dalloc(c, &c->ep_len, N) ||
         dalloc(c, &c->ep_cnt, TW) || dalloc(c, &c->ep_base, TW) || dalloc(c, &c->ep_word, 1);
}

// The table of a collect that counted `total` episodes: the count is checked against the fragment's
// size and the table grown to max(total, 2 * cap) rows when it holds fewer.  The caller has
// synchronized the stream, so nothing in flight reads the old table.
int ep_table_fit(ddrl_ctx* c, long long total) {
  if (total < 0 || total > (long long)c->cfg.frag_len * c->cfg.n_envs) return fail("episodes: bad episode count");
  if (total > c->ep_cap) {
    const long long cap = std::max(total, 2 * c->ep_cap);
    dfree(c, &c->ep_table);
    c->ep_cap = 0;
    c->ep_rows = -1;
    if (dalloc(c, &c->ep_table, (size_t)cap * 8)) return -1;
    c->ep_cap = cap;
  }
  return 0;
}
}  // namespace ddrl_impl

extern "C" {

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
  if (ep_table_fit(c, total)) return -1;
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

}  // extern "C"
