// Device env plane: the QuAntruped stand-in of the host env plane (hostenv.cpp) stepped by a
// kernel.  The dynamics are envdyn.h's, the source the host plane runs too; this file only maps
// them onto lanes and onto the struct-of-arrays state.
//
// Arithmetic contract: no contraction (the host build never fuses a * b + c; HIP's default
// would), no fast-math, fp64 sin / cos of the device library.  Everything but sin / cos then
// matches the host bit for bit.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "common.h"
#include "envdyn.h"
#include "kernels.h"

using namespace envdyn;

namespace {

__device__ __forceinline__ EnvState load_state(const DevEnvArgs& A, int e) {
  const size_t N = A.N;
  double p[kStateDoubles];
#pragma unroll
  for (int f = 0; f < 38; ++f) p[f] = A.st[f * N + e];
  p[38] = 0.0; p[39] = 0.0;
  p[40] = A.st[38 * N + e];
  EnvState s;
  unpack_state(p, s);
  s.steps = A.steps[e];
  s.episode = A.episode[e];
  return s;
}

__device__ __forceinline__ void store_state(const DevEnvArgs& A, int e, const EnvState& s) {
  const size_t N = A.N;
  double p[kStateDoubles];
  pack_state(s, p);
#pragma unroll
  for (int f = 0; f < 38; ++f) A.st[f * N + e] = p[f];
  A.st[38 * N + e] = p[40];
  A.steps[e] = s.steps;
  A.episode[e] = s.episode;
}

__device__ __forceinline__ Terrain terrain_of(const DevEnvArgs& A) {
  return Terrain{A.ter_lo, A.ter_hi, A.ter_bump, A.ter_inv_bump, A.ter_gen};
}

// the value lane k of the quad holds, in every lane of the quad (quad_perm [k, k, k, k])
template <int K>
__device__ __forceinline__ double quad_get(double v) { return dpp_mov_d<K * 0x55>(v); }

// Four lanes per env, lane `leg` of the quad owns leg `leg` (its hip and knee joint, its foot).
// Per substep a lane computes its leg's contact force and push, the quad exchanges the four pairs
// with DPP quad moves, every lane sums them in the host's order and integrates the torso (four
// bit-equal copies), and each lane integrates its two joints.  A 64-env block is one 256-thread
// workgroup; quads never straddle a wave, and a quad leaves as a whole when its env is past N.
// The step is a latency-bound chain (five substeps of dependent fp64 sin / cos), so the lanes buy
// a shorter chain, not throughput: 9.1 us per launch at 128 envs and 10.0 us at 4096, against
// 20.5 / 21.6 us for one thread per env running envdyn::step_env, bit-equal to this kernel
// (profiles/devenv/step_ab.json).
//
// kTerrain: the instance for uneven ground.  Each leg lane evaluates the height field under its
// own foot in every substep (envdyn::ground_height: four lattice hashes and the interpolation,
// integer and fp64 ALU work, no memory traffic) ahead of its contact force; what does not depend
// on the point (the field's hash key, the env's smoothness) is formed once per step.  The flat
// instance contains none of it.
//
// kTvEnv: the instance for a per-env velocity table (DevEnvArgs::tv_env): a restarting env takes
// its own entry instead of a draw from the list.  An instance and not a test of the pointer: with
// the test in it the flat kernel measured 0.24 us longer per launch than without
// (profiles/eval/sweep_time.json, DESIGN.md section 3 "Evaluation members").
template <bool kTerrain, bool kTvEnv>
__global__ void __launch_bounds__(256) k_devenv_step(DevEnvArgs A, const float* __restrict__ actions) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int e = g >> 2, leg = g & 3;
  if (e >= A.N) return;
  const size_t N = A.N;
  double* const st = A.st + e;
  const int hip = 2 * leg, knee = hip + 1;
  Torso t{st[0 * N], st[1 * N], st[2 * N], st[3 * N], st[4 * N], st[5 * N], st[6 * N], st[7 * N], st[8 * N], st[9 * N]};
  double q_h = st[(10 + hip) * N], q_k = st[(10 + knee) * N];
  double qd_h = st[(18 + hip) * N], qd_k = st[(18 + knee) * N];
  double frc_h = 0.0, frc_k = 0.0;
  double tv = st[38 * N];
  int steps = A.steps[e];
  unsigned episode = A.episode[e];
  const double a_h = clip_action(actions[(size_t)e * 8 + hip]), a_k = clip_action(actions[(size_t)e * 8 + knee]);
  const double x0 = t.x;
  double force = 0.0, f0 = 0.0, f1 = 0.0, f2 = 0.0, f3 = 0.0;
  Ground ground{0, 0.0, 0.0};
  if constexpr (kTerrain) ground = ground_of(terrain_of(A), A.seed, e, episode);
#pragma unroll 1
  for (int f = 0; f < kFrameSkip; ++f) {
    double push;
    if constexpr (kTerrain) leg_contact_on(ground, leg, t.x, t.y, t.z, t.vz, q_h, q_k, qd_h, force, push);
    else leg_contact(t.z, t.vz, q_h, q_k, qd_h, force, push);
    f0 = quad_get<0>(force); f1 = quad_get<1>(force); f2 = quad_get<2>(force); f3 = quad_get<3>(force);
    const double p0 = quad_get<0>(push), p1 = quad_get<1>(push), p2 = quad_get<2>(push), p3 = quad_get<3>(push);
    LegSums sums = leg_sums_zero();
    accum_leg(sums, 0, f0, p0);
    accum_leg(sums, 1, f1, p1);
    accum_leg(sums, 2, f2, p2);
    accum_leg(sums, 3, f3, p3);
    joint_step(hip, a_h, q_h, qd_h, frc_h);
    joint_step(knee, a_k, q_k, qd_k, frc_k);
    torso_step(t, sums);
  }
  ++steps;
  const bool d = unhealthy(t.z) || steps >= A.time_limit;

  // outputs of the step, before a done env is reset.  cfrc [14][6]: lane `leg` writes the three
  // body rows of its leg (hip, leg: zero; foot), and three of the twelve floats of the floor and
  // torso rows; the torso row's last column, the fp32 sum over the legs in leg order, is lane 3's
  float* cf = A.cfrc + (size_t)e * 84;
  float* mine = cf + (2 + 3 * leg) * 6;
#pragma unroll
  for (int i = 0; i < 18; ++i) mine[i] = 0.f;
  foot_row(force, q_h, mine[12], mine[15], mine[17]);
  float share = 0.f;
  if (leg == 3) {
    share += torso_share(f0);
    share += torso_share(f1);
    share += torso_share(f2);
    share += torso_share(f3);
  }
  cf[3 * leg] = 0.f;
  cf[3 * leg + 1] = 0.f;
  cf[3 * leg + 2] = share;
  float* kn = A.kin + (size_t)e * 9;
  kn[1 + hip] = (float)qd_h;
  kn[1 + knee] = (float)qd_k;
  if (leg == 0) {
    kn[0] = (float)(t.x - x0);
    A.fw[e] = forward_reward(t.x, x0, tv, A.D);
    A.done[e] = d ? 1 : 0;
  }

  // a done env starts its next episode at once: every lane redraws the torso (the same bits),
  // its own two joints and the target velocity
  double c_h = a_h, c_k = a_k;
  if (d) {
    episode += 1;
    steps = 0;
    if constexpr (kTvEnv) tv = A.tv_env[e];
    else tv = draw_tv(A.seed, e, episode, A.tv_list, A.n_tv);
    t = Torso{0.0, 0.0, reset_z(A.seed, e, episode), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    q_h = reset_q(A.seed, e, episode, hip); q_k = reset_q(A.seed, e, episode, knee);
    qd_h = reset_qd(A.seed, e, episode, hip); qd_k = reset_qd(A.seed, e, episode, knee);
    frc_h = 0.0; frc_k = 0.0; force = 0.0;
    c_h = 0.0; c_k = 0.0;
  }

  // the observation: one of the quaternion's four sin / cos per lane, exchanged like the forces
  const double half = 0.5 * (leg < 2 ? t.roll : t.pitch);
  const double trig = (leg & 1) ? sin(half) : cos(half);
  double w[4];
  quat_of(quad_get<0>(trig), quad_get<1>(trig), quad_get<2>(trig), quad_get<3>(trig), w);
  float* o = A.obs + (size_t)e * A.D;
  o[kObsQ + hip] = (float)q_h; o[kObsQ + knee] = (float)q_k;
  o[kObsQd + hip] = (float)qd_h; o[kObsQd + knee] = (float)qd_k;
  o[kObsFrc + hip] = (float)frc_h; o[kObsFrc + knee] = (float)frc_k;
  o[kObsCtrl + hip] = (float)c_h; o[kObsCtrl + knee] = (float)c_k;
  if (leg == 0) {
    o[0] = (float)t.z; o[1] = (float)w[0]; o[2] = (float)w[1];
  } else if (leg == 1) {
    o[3] = (float)w[2]; o[4] = (float)w[3]; o[kObsVel] = (float)t.vx;
  } else if (leg == 2) {
    o[kObsVel + 1] = (float)t.vy; o[kObsVel + 2] = (float)t.vz; o[kObsVel + 3] = (float)t.wroll;
  } else {
    o[kObsVel + 4] = (float)t.wpitch; o[kObsVel + 5] = (float)0.0;
    if (A.D > 43) o[kObsTv] = (float)tv;
  }

  // the state: own joints and foot; the torso's ten fields, tv and the counters split over the quad
  st[(10 + hip) * N] = q_h; st[(10 + knee) * N] = q_k;
  st[(18 + hip) * N] = qd_h; st[(18 + knee) * N] = qd_k;
  st[(26 + hip) * N] = frc_h; st[(26 + knee) * N] = frc_k;
  st[(34 + leg) * N] = force;
  const double tf[10] = {t.x, t.y, t.z, t.vx, t.vy, t.vz, t.roll, t.pitch, t.wroll, t.wpitch};
  if (leg == 0) {
    st[0 * N] = tf[0]; st[4 * N] = tf[4]; st[8 * N] = tf[8];
  } else if (leg == 1) {
    st[1 * N] = tf[1]; st[5 * N] = tf[5]; st[9 * N] = tf[9];
  } else if (leg == 2) {
    st[2 * N] = tf[2]; st[6 * N] = tf[6]; st[38 * N] = tv;
  } else {
    st[3 * N] = tf[3]; st[7 * N] = tf[7];
    A.steps[e] = steps;
    A.episode[e] = episode;
  }
}

// reset_all / reset_episodes / reset_state of the host plane (hostenv.h), one thread per env
__global__ void __launch_bounds__(64) k_devenv_reset(DevEnvArgs A, int mode) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= A.N) return;
  EnvState s = load_state(A, e);
  if (mode == DEVENV_RESET_ALL) s.episode = 0;
  reset_env(s, A.seed, e, mode != DEVENV_RESET_STATE, A.tv_list, A.n_tv);
  if (A.tv_env && mode != DEVENV_RESET_STATE) s.tv = A.tv_env[e];   // the env's fixed velocity, not the draw
  if (mode == DEVENV_RESET_ALL) s.steps = stagger_steps(A.seed, e, A.time_limit);
  if (mode != DEVENV_RESET_STATE) {
    write_obs(s, A.obs + (size_t)e * A.D, A.D, nullptr);
    A.done[e] = 0;
  }
  store_state(A, e, s);
}

__global__ void __launch_bounds__(64) k_devenv_pack(DevEnvArgs A, double* packed, int unpack) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= A.N) return;
  double* p = packed + (size_t)e * kStateDoubles;
  if (unpack) {
    EnvState s;
    unpack_state(p, s);
    store_state(A, e, s);
  } else {
    pack_state(load_state(A, e), p);
  }
}

// the probe of the height field: one thread per point
__global__ void __launch_bounds__(64) k_devenv_terrain_height(DevEnvArgs A, const int* __restrict__ env_index,
                                                              const double* __restrict__ xy, int n,
                                                              double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int e = env_index[i];
  if (e < 0 || e >= A.N) {   // the indices are in device memory, unseen by the host: NaN, and no read past the arrays
    out[i] = __builtin_nan("");
    return;
  }
  out[i] = ground_height(ground_of(terrain_of(A), A.seed, e, A.episode[e]), xy[2 * (size_t)i], xy[2 * (size_t)i + 1]);
}

}  // namespace

void launch_devenv_step(hipStream_t s, const DevEnvArgs& a, const float* actions) {
  const dim3 grid((4 * a.N + 255) / 256);
  if (a.tv_env) {
    if (a.ter_on) hipLaunchKernelGGL((k_devenv_step<true, true>), grid, dim3(256), 0, s, a, actions);
    else hipLaunchKernelGGL((k_devenv_step<false, true>), grid, dim3(256), 0, s, a, actions);
  } else {
    if (a.ter_on) hipLaunchKernelGGL((k_devenv_step<true, false>), grid, dim3(256), 0, s, a, actions);
    else hipLaunchKernelGGL((k_devenv_step<false, false>), grid, dim3(256), 0, s, a, actions);
  }
}

void launch_devenv_terrain_height(hipStream_t s, const DevEnvArgs& a, const int* env_index, const double* xy, int n,
                                  double* out) {
  if (n < 1) return;
  hipLaunchKernelGGL(k_devenv_terrain_height, dim3((n + 63) / 64), dim3(64), 0, s, a, env_index, xy, n, out);
}

void launch_devenv_reset(hipStream_t s, const DevEnvArgs& a, int mode) {
  hipLaunchKernelGGL(k_devenv_reset, dim3((a.N + 63) / 64), dim3(64), 0, s, a, mode);
}

void launch_devenv_pack(hipStream_t s, const DevEnvArgs& a, double* packed, int unpack) {
  hipLaunchKernelGGL(k_devenv_pack, dim3((a.N + 63) / 64), dim3(64), 0, s, a, packed, unpack);
}
