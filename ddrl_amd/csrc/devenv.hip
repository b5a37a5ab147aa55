// Device env plane: the QuAntruped stand-in of the host env plane (hostenv.cpp) stepped by a
// kernel.  The dynamics are envdyn.h's, the source the host plane runs too; this file only maps
// them onto lanes and onto the struct-of-arrays state.
//
// Arithmetic contract: no contraction (the host build never fuses a * b + c; HIP's default
// would), no fast-math, fp64 sin / cos of the device library.  Everything but sin / cos then
// matches the host bit for bit.
//
// The step kernel's body is a text of its own (devenv_step_body.h), included inside the kernel's braces
// here and, below the same pragma, in rollout_group.hip's member-axis kernel; it reads A and actions.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "common.h"
#include "envdyn.h"
#include "kernels.h"
#include "devenv_step.h"

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
#include "devenv_step_body.h"
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
