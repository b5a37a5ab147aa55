// f1: host env plane -- the clean-room vectorized QuAntruped stand-in and its thread pool
// (see hostenv.h), plus the C-ABI to create / reset / step it.  The pipelined rollout over
// it (ddrl_rollout_hostenv) lives in capi_rollout.cpp next to the context it drives.
#include "hostenv.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/ddrl_hip.h"

namespace hostenv {

Pool::Pool(int n_threads) {
  for (int i = 1; i < std::max(1, n_threads); ++i) workers_.emplace_back([this, i] { run(i); });
}

Pool::~Pool() {
  {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
  }
  cv_.notify_all();
  for (auto& t : workers_) t.join();
}

void Pool::run(int) {
  // A worker takes chunks only of the generation it woke up for: a worker still looping after
  // the last chunk of generation g was finished must not pick up a chunk of g + 1 with g's job
  // (the caller's function object is gone by then).
  uint64_t seen = 0;
  std::unique_lock<std::mutex> lk(mu_);
  for (;;) {
    cv_.wait(lk, [&] { return stop_ || generation_ != seen; });
    if (stop_) return;
    seen = generation_;
    const std::function<void(int, int)>* job = job_;
    while (generation_ == seen && next_ < chunks_) {
      const int c = next_++, n = n_, ch = chunks_;
      lk.unlock();
      (*job)((int)((long long)n * c / ch), (int)((long long)n * (c + 1) / ch));
      lk.lock();
      if (++finished_ == ch) done_cv_.notify_all();
    }
  }
}

void Pool::parallel_for(int n, const std::function<void(int, int)>& fn) {
  if (n <= 0) return;
  if (workers_.empty()) {
    fn(0, n);
    return;
  }
  {
    std::lock_guard<std::mutex> lk(mu_);
    job_ = &fn;
    n_ = n;
    chunks_ = std::min(n, 4 * size());
    next_ = 0;
    finished_ = 0;
    ++generation_;
  }
  cv_.notify_all();
  for (;;) {   // the caller works too
    int c;
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (next_ >= chunks_) break;
      c = next_++;
    }
    const int lo = (int)((long long)n * c / chunks_), hi = (int)((long long)n * (c + 1) / chunks_);
    fn(lo, hi);
    std::lock_guard<std::mutex> lk(mu_);
    if (++finished_ == chunks_) done_cv_.notify_all();
  }
  std::unique_lock<std::mutex> lk(mu_);
  done_cv_.wait(lk, [&] { return finished_ == chunks_; });
  job_ = nullptr;
}

}  // namespace hostenv

using hostenv::EnvState;

// The dynamics are envdyn.h's, shared with the device plane (devenv.hip).
void ddrl_hostenv::reset_env(int e, bool draw_tv) {
  envdyn::reset_env(st[e], seed, e, draw_tv, tv_list.data(), (int)tv_list.size());
}

void ddrl_hostenv::write_obs(int e, const double* ctrl) { envdyn::write_obs(st[e], obs + (size_t)e * D, D, ctrl); }

void ddrl_hostenv::step_env(int e, const float* a8) {
  envdyn::step_env(st[e], a8, obs + (size_t)e * D, fw + e, cfrc + (size_t)e * 14 * 6, kin + (size_t)e * 9, done + e, D,
                   time_limit, seed, e, tv_list.data(), (int)tv_list.size(),
                   envdyn::terrain_on(terrain) ? &terrain : nullptr);
}

void ddrl_hostenv::state_get(double* out) const {
  for (int e = 0; e < N; ++e) envdyn::pack_state(st[e], out + (size_t)e * envdyn::kStateDoubles);
}

void ddrl_hostenv::state_set(const double* in) {
  for (int e = 0; e < N; ++e) envdyn::unpack_state(in + (size_t)e * envdyn::kStateDoubles, st[e]);
}

void ddrl_hostenv::reset_all() {
  pool->parallel_for(N, [this](int lo, int hi) {
    for (int e = lo; e < hi; ++e) {
      st[e].episode = 0;
      reset_env(e);
      // staggered episode phases, like a long-running sampler (the synthetic rollouts too)
      st[e].steps = envdyn::stagger_steps(seed, e, time_limit);
      write_obs(e, nullptr);
      done[e] = 0;
    }
  });
}

void ddrl_hostenv::reset_state() {
  pool->parallel_for(N, [this](int lo, int hi) {
    for (int e = lo; e < hi; ++e) reset_env(e, false);   // steps = 0: the TimeLimit count restarts too
  });
}

void ddrl_hostenv::reset_episodes() {
  pool->parallel_for(N, [this](int lo, int hi) {
    for (int e = lo; e < hi; ++e) {
      reset_env(e);
      write_obs(e, nullptr);
      done[e] = 0;
    }
  });
}

void ddrl_hostenv::step(int e0, int e1) {
  pool->parallel_for(e1 - e0, [this, e0](int lo, int hi) {
    for (int e = e0 + lo; e < e0 + hi; ++e) step_env(e, act + (size_t)e * 8);
  });
}

// ---- C-ABI ------------------------------------------------------------------------------
namespace {
thread_local std::string g_henv_err;
}
extern "C" const char* ddrl_hostenv_last_error(void) { return g_henv_err.c_str(); }

extern "C" int ddrl_hostenv_create(int n_envs, int obs_dim, int n_threads, uint64_t seed, float target_velocity,
                                   ddrl_hostenv** out) {
  if (!out || n_envs < 1 || (obs_dim != 43 && obs_dim != 44) || n_threads < 1 ||
      (obs_dim == 44 && !(target_velocity > 0.f))) {
    g_henv_err = "ddrl_hostenv_create: n_envs >= 1, obs_dim 43 or 44 (44: target_velocity > 0), n_threads >= 1";
    return -1;
  }
  auto* h = new ddrl_hostenv();
  h->N = n_envs;
  h->D = obs_dim;
  h->seed = seed;
  h->tv_list.assign(1, (double)target_velocity);
  h->st.assign(n_envs, EnvState{});
  // the create-time velocity until the first reset draws one (a step before any reset must not
  // divide by zero in the TVel reward)
  for (auto& s : h->st) s.tv = (double)target_velocity;
  const size_t N = n_envs;
  // pinned when a GPU is present (the DMA engines read / write them directly); without one
  // (CPU tests of the env plane) ordinary aligned host memory
  int ndev = 0;
  h->pinned = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
  auto alloc = [&](void** p, size_t bytes) {
    if (h->pinned) return hipHostMalloc(p, bytes, hipHostMallocDefault) == hipSuccess;
    *p = std::aligned_alloc(64, (bytes + 63) / 64 * 64);
    return *p != nullptr;
  };
  if (!alloc((void**)&h->obs, N * obs_dim * 4) || !alloc((void**)&h->act, N * 8 * 4) || !alloc((void**)&h->fw, N * 4) ||
      !alloc((void**)&h->cfrc, N * 14 * 6 * 4) || !alloc((void**)&h->done, N) || !alloc((void**)&h->kin, N * 9 * 4)) {
    g_henv_err = "ddrl_hostenv_create: host buffer allocation failed";
    ddrl_hostenv_destroy(h);
    return -1;
  }
  std::memset(h->act, 0, N * 8 * 4);
  std::memset(h->kin, 0, N * 9 * 4);
  h->pool = new hostenv::Pool(n_threads);
  *out = h;
  return 0;
}

extern "C" int ddrl_hostenv_destroy(ddrl_hostenv* h) {
  if (!h) return 0;
  delete h->pool;
  for (void* p : {(void*)h->obs, (void*)h->act, (void*)h->fw, (void*)h->cfrc, (void*)h->done, (void*)h->kin}) {
    if (!p) continue;
    if (h->pinned) (void)hipHostFree(p);
    else std::free(p);
  }
  delete h;
  return 0;
}

extern "C" int ddrl_hostenv_buffers(ddrl_hostenv* h, float** obs, float** act, float** fw, float** cfrc,
                                    uint8_t** done) {
  if (!h) {
    g_henv_err = "null host env";
    return -1;
  }
  if (obs) *obs = h->obs;
  if (act) *act = h->act;
  if (fw) *fw = h->fw;
  if (cfrc) *cfrc = h->cfrc;
  if (done) *done = h->done;
  return 0;
}

extern "C" int ddrl_hostenv_reset(ddrl_hostenv* h) {
  if (!h) {
    g_henv_err = "null host env";
    return -1;
  }
  h->reset_all();
  return 0;
}

extern "C" int ddrl_hostenv_step(ddrl_hostenv* h, int e0, int e1) {
  if (!h || e0 < 0 || e1 > h->N || e0 >= e1) {
    g_henv_err = "ddrl_hostenv_step: bad env range";
    return -1;
  }
  h->step(e0, e1);
  return 0;
}

extern "C" int ddrl_hostenv_threads(ddrl_hostenv* h) { return h ? h->pool->size() : 0; }

extern "C" int ddrl_hostenv_set_target_velocities(ddrl_hostenv* h, const float* list, int n) {
  if (!h || !list || n < 1) {
    g_henv_err = "ddrl_hostenv_set_target_velocities: a list of n >= 1 values";
    return -1;
  }
  for (int i = 0; i < n; ++i) {
    if (h->D > 43 && !(list[i] > 0.f)) {
      g_henv_err = "ddrl_hostenv_set_target_velocities: obs_dim 44 needs target velocities > 0 "
                   "(the TVel reward divides by it)";
      return -1;
    }
  }
  h->tv_list.assign(list, list + n);
  return 0;
}

extern "C" int ddrl_hostenv_target_velocities(ddrl_hostenv* h, float* out, int n) {
  if (!h || !out || n != h->N) {
    g_henv_err = "ddrl_hostenv_target_velocities: out holds n_envs floats";
    return -1;
  }
  for (int e = 0; e < n; ++e) out[e] = (float)h->st[e].tv;
  return 0;
}

extern "C" int ddrl_hostenv_reset_state(ddrl_hostenv* h) {
  if (!h) {
    g_henv_err = "null host env";
    return -1;
  }
  h->reset_state();
  return 0;
}

extern "C" int ddrl_hostenv_set_terrain(ddrl_hostenv* h, double lo, double hi, double bump_scale, uint32_t generation) {
  if (!h) {
    g_henv_err = "null host env";
    return -1;
  }
  if (!(0.0 <= lo && lo <= hi && hi <= 1.0)) {
    g_henv_err = "ddrl_hostenv_set_terrain: smoothness bounds must satisfy 0 <= lo <= hi <= 1";
    return -1;
  }
  if (!(bump_scale > 0.0) || !std::isfinite(bump_scale)) {
    g_henv_err = "ddrl_hostenv_set_terrain: bump_scale must be a finite value > 0";
    return -1;
  }
  h->terrain = envdyn::Terrain{lo, hi, bump_scale, 1.0 / bump_scale, generation};
  return 0;
}

extern "C" int ddrl_hostenv_terrain(ddrl_hostenv* h, double* lo, double* hi, double* bump_scale, uint32_t* generation) {
  if (!h) {
    g_henv_err = "null host env";
    return -1;
  }
  if (lo) *lo = h->terrain.lo;
  if (hi) *hi = h->terrain.hi;
  if (bump_scale) *bump_scale = h->terrain.bump_scale;
  if (generation) *generation = h->terrain.generation;
  return 0;
}

extern "C" int ddrl_hostenv_new_terrain(ddrl_hostenv* h) {
  if (!h) {
    g_henv_err = "null host env";
    return -1;
  }
  ++h->terrain.generation;
  return 0;
}

extern "C" int ddrl_hostenv_terrain_height(ddrl_hostenv* h, const int32_t* env_index, const double* xy, int n,
                                           double* out) {
  if (!h || !env_index || !xy || !out || n < 0) {
    g_henv_err = "ddrl_hostenv_terrain_height: a host env, n >= 0 points (env_index[n], xy[n][2]) and out[n]";
    return -1;
  }
  for (int i = 0; i < n; ++i) {
    if (env_index[i] < 0 || env_index[i] >= h->N) {
      g_henv_err = "ddrl_hostenv_terrain_height: env index out of range";
      return -1;
    }
  }
  h->pool->parallel_for(n, [&](int p0, int p1) {
    for (int i = p0; i < p1; ++i) {
      const int e = env_index[i];
      out[i] = envdyn::ground_height(envdyn::ground_of(h->terrain, h->seed, e, h->st[e].episode), xy[2 * i], xy[2 * i + 1]);
    }
  });
  return 0;
}

extern "C" int ddrl_hostenv_kin(ddrl_hostenv* h, float** kin) {
  if (!h || !kin) {
    g_henv_err = "ddrl_hostenv_kin: null host env / output pointer";
    return -1;
  }
  *kin = h->kin;
  return 0;
}

extern "C" int ddrl_hostenv_set_time_limit(ddrl_hostenv* h, int steps) {
  if (!h || steps < 1) {
    g_henv_err = "ddrl_hostenv_set_time_limit: a host env and steps >= 1";
    return -1;
  }
  h->time_limit = steps;
  return 0;
}

extern "C" int ddrl_hostenv_reset_episodes(ddrl_hostenv* h) {
  if (!h) {
    g_henv_err = "null host env";
    return -1;
  }
  h->reset_episodes();
  return 0;
}

extern "C" int ddrl_hostenv_state_get(ddrl_hostenv* h, double* host, size_t n) {
  if (!h || !host || n != (size_t)h->N * envdyn::kStateDoubles) {
    g_henv_err = "ddrl_hostenv_state_get: a host env and n == n_envs * DDRL_ENV_STATE_DOUBLES doubles";
    return -1;
  }
  h->state_get(host);
  return 0;
}

extern "C" int ddrl_hostenv_state_set(ddrl_hostenv* h, const double* host, size_t n) {
  if (!h || !host || n != (size_t)h->N * envdyn::kStateDoubles) {
    g_henv_err = "ddrl_hostenv_state_set: a host env and n == n_envs * DDRL_ENV_STATE_DOUBLES doubles";
    return -1;
  }
  for (int e = 0; e < h->N; ++e) {
    if (!envdyn::packed_counts_ok(host + (size_t)e * envdyn::kStateDoubles)) {
      g_henv_err = "ddrl_hostenv_state_set: steps and episode must be non-negative integers";
      return -1;
    }
  }
  h->state_set(host);
  return 0;
}
