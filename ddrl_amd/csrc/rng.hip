// Device randomness: the exploration noise of a fragment and the minibatch schedules of an update,
// drawn on the device from a counter-based generator (philox.h) instead of on the host.
//   k_noise_fill:    eps[n_steps][N][n_agents][A] standard normals, one Philox block (four normals,
//                    one 16-byte store) per lane;
//   k_schedule_fill: shuffle[R] and perm[epochs][nb] of every filled policy, each a keyed bijection
//                    computed per element (Feistel network + cycle walking).
// Both are bound by launch overhead and by their stores.  Each has a member instance for a group of
// contexts, the member in blockIdx.z and its operands in a device table; the kernel text is one
// body header per kernel, included by both instances.
#include "common.h"
#include "kernels.h"
#include "philox.h"

#define RNG_THREADS 256
#define RNG_MAX_BLOCKS 2048   // per member (and policy): the rest of the elements by a grid stride

// ---- noise ----
__global__ void __launch_bounds__(RNG_THREADS) k_noise_fill(NoiseMember nm, int n_steps, int N, int B) {
#include "noise_fill_body.h"
}

__global__ void __launch_bounds__(RNG_THREADS) k_noise_fill_group(const NoiseMember* __restrict__ tab, int n_steps, int N, int B) {
  const NoiseMember& nm = tab[blockIdx.z];
#include "noise_fill_body.h"
}

static unsigned rng_blocks(size_t lanes) {
  const size_t b = (lanes + RNG_THREADS - 1) / RNG_THREADS;
  return (unsigned)(b < 1 ? 1 : b > RNG_MAX_BLOCKS ? RNG_MAX_BLOCKS : b);
}

void launch_noise_fill(hipStream_t s, const NoiseMember& nm, int n_steps, int N, int B) {
  hipLaunchKernelGGL(k_noise_fill, dim3(rng_blocks((size_t)n_steps * N * B)), dim3(RNG_THREADS), 0, s, nm, n_steps, N, B);
}

void launch_noise_fill_group(hipStream_t s, const NoiseMember* tab_dev, int M, int n_steps, int N, int B) {
  hipLaunchKernelGGL(k_noise_fill_group, dim3(rng_blocks((size_t)n_steps * N * B), 1, M), dim3(RNG_THREADS), 0, s, tab_dev,
                     n_steps, N, B);
}

// ---- schedules ----
__global__ void __launch_bounds__(RNG_THREADS) k_schedule_fill(ScheduleMember sm, ScheduleShape sh) {
#include "schedule_fill_body.h"
}

__global__ void __launch_bounds__(RNG_THREADS) k_schedule_fill_group(const ScheduleMember* __restrict__ tab, ScheduleShape sh) {
  const ScheduleMember& sm = tab[blockIdx.z];
#include "schedule_fill_body.h"
}

// blocks along x: enough for the longest of the filled policies
static unsigned schedule_blocks(const ScheduleShape& sh) {
  size_t most = 0;
  for (int i = 0; i < sh.n_pol; ++i) {
    const int p = sh.pid[i];
    const size_t n = (size_t)sh.R[p] + (size_t)sh.epochs * sh.nb[p];
    most = n > most ? n : most;
  }
  return rng_blocks(most);
}

void launch_schedule_fill(hipStream_t s, const ScheduleMember& sm, const ScheduleShape& sh) {
  hipLaunchKernelGGL(k_schedule_fill, dim3(schedule_blocks(sh), sh.n_pol), dim3(RNG_THREADS), 0, s, sm, sh);
}

void launch_schedule_fill_group(hipStream_t s, const ScheduleMember* tab_dev, int M, const ScheduleShape& sh) {
  hipLaunchKernelGGL(k_schedule_fill_group, dim3(schedule_blocks(sh), sh.n_pol, M), dim3(RNG_THREADS), 0, s, tab_dev, sh);
}
