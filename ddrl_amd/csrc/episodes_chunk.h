// The chunked record loads and the accumulation of the episode walk: what ep_walk_body.h calls.
// Included at file scope by episodes.hip and finish_group.hip, below their
// `#pragma clang fp contract(off)`.
#pragma once

#define EP_SCAN_THREADS 256

// The record loads of a chunk of EP_U time steps are issued one chunk ahead of the accumulation
// (k_gae's GaeChunk): the table stores may alias them as far as the compiler knows.
#define EP_U 16
struct EpChunk { float r[EP_U][DDRL_MAXAG]; bool d[EP_U]; };

__device__ __forceinline__ void ep_load(const EpArgs& a, const float* const rp[DDRL_MAXAG],
                                        const size_t step[DDRL_MAXAG], int e, int t0, bool valid, EpChunk& ch) {
#pragma unroll
  for (int u = 0; u < EP_U; ++u) {
    const int t = t0 + u;
    ch.d[u] = false;
#pragma unroll
    for (int j = 0; j < DDRL_MAXAG; ++j) ch.r[u][j] = 0.f;
    if (valid && t < a.T) {
#pragma unroll
      for (int j = 0; j < DDRL_MAXAG; ++j)
        if (j < a.n_agents) ch.r[u][j] = rp[j][(size_t)t * step[j]];
      ch.d[u] = a.done_tn[(size_t)t * a.N + e] != 0;
    }
  }
}

struct EpState { double total, ag[DDRL_MAXAG]; int len; };

__device__ __forceinline__ void ep_run(const EpArgs& a, int e, int w, int lane, int t0, const EpChunk& ch,
                                       EpState& st) {
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
  for (int u = 0; u < EP_U; ++u) {
    const int t = t0 + u;
    if (t >= a.T) break;                                  // uniform: the ballot below sees whole waves
#pragma unroll
    for (int j = 0; j < DDRL_MAXAG; ++j)
      if (j < a.n_agents) {
        const double r = (double)ch.r[u][j];
        st.ag[j] += r;
        st.total += r;
      }
    st.len += 1;
    const unsigned long long m = __ballot(ch.d[u]);
    if (ch.d[u]) {
      const long long row = a.base[t * a.W + w] + __popcll(m & ((1ull << lane) - 1ull));
      if (row < a.cap) {                                  // the host sized the table from the scan's total
        double* o = a.table + row * 8;
        o[0] = (double)t; o[1] = (double)e; o[2] = (double)st.len; o[3] = st.total;
#pragma unroll
        for (int j = 0; j < DDRL_MAXAG; ++j) o[4 + j] = j < a.n_agents ? st.ag[j] : nan;
      }
      st.total = 0.0;
#pragma unroll
      for (int j = 0; j < DDRL_MAXAG; ++j) st.ag[j] = 0.0;
      st.len = 0;
    }
  }
}
