// C-ABI of libddrl_hip.so: the device env plane (devenv.hip) and the fragment that steps it.
#include "ctx.h"

template <class T>
static bool env_alloc(ddrl_devenv* e, T** p, size_t count) {
  void* ptr = nullptr;
  if (dev_zalloc(&ptr, count * sizeof(T)) != hipSuccess) return false;
  e->allocs.push_back(ptr);
  *p = static_cast<T*>(ptr);
  return true;
}

static int chk_env(const ddrl_devenv* e) {
  if (!e) return fail("null device env");
  if (!e->ctx) return fail("device env: its context has been destroyed");
  return 0;
}
#define CHK_ENV(e) \
  if (chk_env(e)) return -1

namespace ddrl_impl {
int chk_env_of(const ddrl_ctx* c, const ddrl_devenv* e) {
  if (chk_env(e)) return -1;
  if (e->ctx != c) return fail("device env belongs to another context");
  return 0;
}
}  // namespace ddrl_impl

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

extern "C" {

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
  const bool stale = c->rgd_env != e->id || c->rgd_gen != e->gen || c->rgd_eps != eps_dev;
  if (graph_run(c, &c->rgd_exec, stale, [&] { return devenv_launches(c, e, eps_dev); })) return -1;
  if (stale) { c->rgd_env = e->id; c->rgd_gen = e->gen; c->rgd_eps = eps_dev; }
  rollout_ran(c);   // what the replayed calls would have noted on the host
  return 0;
}

}  // extern "C"
