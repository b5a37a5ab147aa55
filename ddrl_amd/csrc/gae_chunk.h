// The chunked record loads and the recursion of the GAE scan: what gae_body.h calls.  Included at
// file scope by gae.hip and finish_group.hip, below their `#pragma clang fp contract(off)`.
#pragma once

// The record loads of a chunk of GAE_U time steps are issued one chunk ahead of the
// recursion (the stores of adv / vt may alias them as far as the compiler knows, so it would
// otherwise wait for every load in turn: one memory round trip per time step).
#define GAE_U 16
struct GaeChunk { float v[GAE_U], r[GAE_U]; bool d[GAE_U]; };

__device__ __forceinline__ void gae_load(const GaeArgs& g, int c, int e, int t0, GaeChunk& ch) {
#pragma unroll
  for (int u = 0; u < GAE_U; ++u) {
    const int t = t0 - u;
    if (t >= 0) {
      const float* rp = g.rec + ((size_t)t * g.C + c) * g.lay.stride;
      ch.v[u] = rp[g.lay.vf];
      ch.r[u] = rp[g.lay.rew];
      ch.d[u] = g.done_tn[(size_t)t * g.N + e] != 0;
    }
  }
}

__device__ __forceinline__ void gae_run(const GaeArgs& g, int c, int t0, const GaeChunk& ch, double& acc,
                                        double& nextv, double& s1, double& s2) {
  const double gl = g.gamma * g.lambda_;
#pragma unroll
  for (int u = 0; u < GAE_U; ++u) {
    const int t = t0 - u;
    if (t < 0) break;
    if (ch.d[u]) {
      acc = 0.0;
      nextv = 0.0;
    }
    const double v = (double)ch.v[u];
    const double delta = (double)ch.r[u] + g.gamma * nextv - v;
    acc = delta + gl * acc;
    const float a32 = (float)acc;
    float* rp = g.rec + ((size_t)t * g.C + c) * g.lay.stride;
    rp[g.lay.adv] = a32;
    rp[g.lay.vt] = (float)(acc + v);
    s1 += (double)a32;
    s2 += (double)a32 * (double)a32;
    nextv = v;
  }
}
