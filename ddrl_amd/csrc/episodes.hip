// Episode accounting of the training rollout: the returns and lengths of the episodes that
// finish in a fragment, as RLlib 1.0 counts them.
//
// RLlib MultiAgentEpisode._add_agent_rewards: for every env step, for every agent in agent order,
//   agent_rewards[(agent, policy)] += r;  total_reward += r      (Python floats: fp64),
// length counts env steps, and the step that raises done belongs to the episode it ends.  The
// total is an interleaved sum, not the sum of the per-agent totals.  An episode spans several
// fragments, so the running sums of every env stay in the context between calls.
//
// The reward added is the fp32 `rew` field of the agent's record (what the learner trains on),
// widened to fp64.  Agent j of env e is row c = e * k_p + slot of policy p = policy_of_agent[j],
// the mapping k_reward writes with.
//
// Output: one row of 8 doubles (a 64-byte line) per finished episode,
//   {t, env, length, total, agent_0 .. agent_3}   (agents the env does not have: NaN),
// in ascending (t, env) order.  The row position is counts + an exclusive scan + the rank of the
// lane in its wave's ballot: nothing depends on timing, and there is no atomic of any kind.
//   k_ep_count: cnt[t][w] = popcount of the ballot of done_tn[t][64 w .. 64 w + 63];
//   k_ep_scan:  base = exclusive scan of cnt in (t, w) order (one workgroup), total to a word;
//   k_ep_walk:  one thread per env, one wave per 64 consecutive envs, forward over t.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

__global__ void __launch_bounds__(256) k_ep_count(EpArgs a) {
  const int gw = (blockIdx.x * 256 + threadIdx.x) >> 6;   // wave = (t, w)
  const int lane = threadIdx.x & 63;
  if (gw >= a.T * a.W) return;                             // whole waves leave together
  const int t = gw / a.W, w = gw - t * a.W;
  const int e = w * 64 + lane;
  const bool d = e < a.N && a.done_tn[(size_t)t * a.N + e] != 0;
  const unsigned long long m = __ballot(d);
  if (lane == 0) a.cnt[gw] = __popcll(m);
}

// Exclusive scan of n = T * W counts by one workgroup: every thread sums a contiguous run,
// thread 0 scans the 256 run totals, every thread writes its run's bases.
#define EP_SCAN_THREADS 256
__global__ void __launch_bounds__(EP_SCAN_THREADS) k_ep_scan(EpArgs a) {
  __shared__ long long part[EP_SCAN_THREADS];
  const int n = a.T * a.W;
  const int per = (n + EP_SCAN_THREADS - 1) / EP_SCAN_THREADS;
  const int i0 = min(n, (int)threadIdx.x * per), i1 = min(n, i0 + per);
  long long s = 0;
  for (int i = i0; i < i1; ++i) s += a.cnt[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long run = 0;
    for (int i = 0; i < EP_SCAN_THREADS; ++i) {
      const long long v = part[i];
      part[i] = run;
      run += v;
    }
    a.total[0] = run;
  }
  __syncthreads();
  long long run = part[threadIdx.x];
  for (int i = i0; i < i1; ++i) {
    a.base[i] = run;
    run += a.cnt[i];
  }
}

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

__global__ void __launch_bounds__(64) k_ep_walk(EpArgs a) {
  const int w = blockIdx.x, lane = threadIdx.x;
  const int e = w * 64 + lane;
  const bool valid = e < a.N;
  const float* rp[DDRL_MAXAG];
  size_t step[DDRL_MAXAG];
#pragma unroll
  for (int j = 0; j < DDRL_MAXAG; ++j) {
    rp[j] = nullptr;
    step[j] = 0;
    if (j < a.n_agents && valid) {
      const int p = a.policy_of_agent[j];
      const size_t C = (size_t)a.N * a.k[p];
      step[j] = C * a.lay[p].stride;
      rp[j] = a.rec[p] + ((size_t)e * a.k[p] + a.slot_of_agent[j]) * a.lay[p].stride + a.lay[p].rew;
    }
  }
  EpState st;
  st.total = 0.0;
  st.len = 0;
#pragma unroll
  for (int j = 0; j < DDRL_MAXAG; ++j) st.ag[j] = 0.0;
  if (valid) {
    st.total = a.ep_total[e];
    st.len = a.ep_len[e];
#pragma unroll
    for (int j = 0; j < DDRL_MAXAG; ++j) st.ag[j] = a.ep_agent[(size_t)e * DDRL_MAXAG + j];
  }
  const int nch = (a.T + EP_U - 1) / EP_U;
  EpChunk ca, cb;
  ep_load(a, rp, step, e, 0, valid, ca);
  for (int k = 0; k < nch; k += 2) {
    const int ta = k * EP_U, tb = ta + EP_U;
    if (k + 1 < nch) ep_load(a, rp, step, e, tb, valid, cb);
    ep_run(a, e, w, lane, ta, ca, st);
    if (k + 1 >= nch) break;
    if (k + 2 < nch) ep_load(a, rp, step, e, tb + EP_U, valid, ca);
    ep_run(a, e, w, lane, tb, cb, st);
  }
  if (valid) {
    a.ep_total[e] = st.total;
    a.ep_len[e] = st.len;
#pragma unroll
    for (int j = 0; j < DDRL_MAXAG; ++j) a.ep_agent[(size_t)e * DDRL_MAXAG + j] = st.ag[j];
  }
}

void launch_ep_count_scan(hipStream_t s, const EpArgs& a) {
  const int waves = a.T * a.W;
  hipLaunchKernelGGL(k_ep_count, dim3((waves + 3) / 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_ep_scan, dim3(1), dim3(EP_SCAN_THREADS), 0, s, a);
}

void launch_ep_walk(hipStream_t s, const EpArgs& a) {
  hipLaunchKernelGGL(k_ep_walk, dim3(a.W), dim3(64), 0, s, a);
}
