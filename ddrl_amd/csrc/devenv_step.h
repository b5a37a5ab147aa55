// What the env-step text (devenv_step_body.h) calls besides envdyn.h.  Included at file scope after common.h,
// kernels.h and envdyn.h, none of which it includes: the unit places envdyn.h below its contraction pragma.
#pragma once

__device__ __forceinline__ envdyn::Terrain terrain_of(const DevEnvArgs& A) {
  return envdyn::Terrain{A.ter_lo, A.ter_hi, A.ter_bump, A.ter_inv_bump, A.ter_gen};
}

// the value lane k of the quad holds, in every lane of the quad (quad_perm [k, k, k, k])
template <int K>
__device__ __forceinline__ double quad_get(double v) { return dpp_mov_d<K * 0x55>(v); }
