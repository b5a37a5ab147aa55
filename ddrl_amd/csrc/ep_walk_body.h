// The text of k_ep_walk (episodes.hip) and k_ep_walk_group (finish_group.hip), included inside the
// kernel's braces.  Operands: a, the EpArgs as ep_load / ep_run read it (N, T, W, n_agents, done_tn,
// base, the in-flight state, table, cap), and the per-policy tables behind accessor macros, which a
// group reads from its by-value arguments and its member's table entry:
//   EP_POLICY_OF(j), EP_SLOT_OF(j): agent j's policy and slot;  EP_K(p), EP_LAY(p), EP_REC(p).
// blockIdx.x is the wave of 64 envs.  Nothing in front of the chunk loop leaves early: ep_run's
// ballot needs whole waves.
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
      const int p = EP_POLICY_OF(j);
      const size_t C = (size_t)a.N * EP_K(p);
      step[j] = C * EP_LAY(p).stride;
      rp[j] = EP_REC(p) + ((size_t)e * EP_K(p) + EP_SLOT_OF(j)) * EP_LAY(p).stride + EP_LAY(p).rew;
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
