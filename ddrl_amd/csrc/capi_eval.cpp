// C-ABI of libddrl_hip.so: evaluation of the context's policies (eval.hip, eval_members.hip, eval_sens.hip).
#include "ctx.h"

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

extern "C" {

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
  if (dgrow(c, &c->ev_table, &c->ev_table_E, E, N * 6)) return -1;
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
  CHK_PID(c, policy);
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

// What the loops of ddrl_eval_hostenv and ddrl_eval_devenv share.  Their arguments, and the steps to run at the most:
static int eval_loop_limit(const float* eps_dev, int eps_steps, int max_steps, int poll_every, int* limit) {
  if (max_steps < 1 || poll_every < 1) return fail("evaluation: max_steps and poll_every must be >= 1");
  if (eps_dev && eps_steps < 1) return fail("evaluation: eps_steps must be >= 1 with a noise buffer");
  *limit = eps_dev ? std::min(max_steps, eps_steps) : max_steps;
  return 0;
}

// ... and the poll after step t: every poll_every steps, *stop when all envs have finished
static int eval_loop_poll(ddrl_ctx* c, int t, int poll_every, bool* stop) {
  if (t % poll_every) return 0;
  int64_t eps_done = 0, fin = 0;
  if (ddrl_eval_progress(c, &eps_done, &fin)) return -1;
  *stop = fin == (int64_t)c->cfg.n_envs;
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
  int limit = 0;
  if (eval_loop_limit(eps_dev, eps_steps, max_steps, poll_every, &limit)) return -1;
  const size_t N = g.n_envs, D = g.obs_full_dim;
  const size_t eps_step = N * g.n_agents * g.act_dim;
  env->reset_episodes();
  int rc = h2d(c, c->h_obs, env->obs, N * D * 4);
  int t = 0;
  bool stop = false;
  for (; t < limit && !rc && !stop;) {
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
    rc = rc || eval_loop_poll(c, t, poll_every, &stop);
  }
  // the pinned buffers are the caller's again only once the stream has consumed them
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail("stream synchronize failed");
  if (steps_run) *steps_run = t;
  return rc ? -1 : 0;
}

int ddrl_eval_devenv(ddrl_ctx* c, ddrl_devenv* e, const float* eps_dev, int eps_steps, int max_steps, int poll_every,
                     int* steps_run) {
  CHK_EVAL(c);
  if (chk_env_of(c, e)) return -1;
  const ddrl_cfg& g = c->cfg;
  int limit = 0;
  if (eval_loop_limit(eps_dev, eps_steps, max_steps, poll_every, &limit)) return -1;
  const size_t eps_step = (size_t)g.n_envs * g.n_agents * g.act_dim;
  int rc = ddrl_devenv_reset_episodes(e);
  int t = 0;
  bool stop = false;
  for (; t < limit && !rc && !stop;) {
    rc = ddrl_eval_act(c, e->a.obs, eps_dev ? eps_dev + (size_t)t * eps_step : nullptr, c->h_act, nullptr);
    if (!rc && c->sens_on) rc = ddrl_eval_sens(c, e->a.obs, nullptr);
    rc = rc || ddrl_devenv_step(e, c->h_act) || ddrl_eval_step(c, e->a.fw, e->a.cfrc, c->h_act, e->a.kin, e->a.done);
    if (rc) break;
    ++t;
    rc = eval_loop_poll(c, t, poll_every, &stop);
  }
  if (steps_run) *steps_run = t;
  return rc ? -1 : 0;
}

}  // extern "C"
