// a11 / a12: GAE reverse scan over a time-major fragment, fused with the
// standardization statistics of the advantages.
//
// RLlib 1.0 compute_advantages (postprocess_ppo_gae, run once per agent trajectory segment):
//   delta_t = r_t + gamma * V_{t+1} - V_t, with V_T = last_r (0 after done, else V(s_T));
//   adv = lfilter([1], [1, -gamma*lambda], delta[::-1])[::-1]  in float64,
//   value_targets = float32(adv + vf_preds), adv = float32(adv).
// A fragment is split into episode segments at done flags; within one chain the
// recursion y_t = delta_t + gamma*lambda*y_{t+1} (reset after a done) is exactly lfilter's.
// One thread per chain; the loads over t are coalesced across chains (time-major rows).
// StandardizeFields: (adv - mean) / max(1e-4, std) over the policy's whole batch; the sums
// are fp64 and reduced in a fixed order (per-wave partials + one finalize block per policy).
//
// The kernel bodies are texts of their own (gae_body.h, gae_finalize_body.h; the chunk helpers in
// gae_chunk.h), included inside the braces here and in finish_group.hip, which runs them with a
// member axis.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "gae_chunk.h"

// One launch for all policies (blockIdx.y), one wave per block: a policy's C chains spread
// over C / 64 workgroups (Local at 4096 envs: 256 CUs busy instead of 16, whose texture units
// serialized the strided record loads; 4 x 255 -> one ~60 us launch).  Each block writes its
// wave's (sum adv, sum adv^2); the finalize sums them four at a time as ((w0 + w1) + (w2 + w3))
// and then over the groups in order -- the 256-thread reduction's order, so adv_norm and the
// totals are bit-identical to it.
__global__ void __launch_bounds__(64) k_gae(GaeBatch gb) {
  const GaeArgs& g = gb.g[blockIdx.y];
#include "gae_body.h"
}

__global__ void k_gae_finalize(GaeBatch gb) {
  if (threadIdx.x != 0) return;
  const GaeArgs& g = gb.g[blockIdx.x];
#include "gae_finalize_body.h"
}

void launch_gae(hipStream_t s, const GaeBatch& gb) {
  int maxw = 1;
  for (int p = 0; p < gb.P; ++p) maxw = maxw > (gb.g[p].C + 63) / 64 ? maxw : (gb.g[p].C + 63) / 64;
  hipLaunchKernelGGL(k_gae, dim3(maxw, gb.P), dim3(64), 0, s, gb);
  hipLaunchKernelGGL(k_gae_finalize, dim3(gb.P), dim3(64), 0, s, gb);
}
