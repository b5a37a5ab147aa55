// The text of k_gae (gae.hip) and k_gae_group (finish_group.hip), included inside the kernel's
// braces.  Operand: g, the GaeArgs of this block's policy (blockIdx.y).  blockIdx.x counts the
// policy's waves of 64 chains.
  if ((int)blockIdx.x * 64 >= g.C) return;
  const int c = blockIdx.x * 64 + threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  if (c < g.C) {
    const int e = c / g.k;
    double acc = 0.0;
    double nextv = (double)g.last_v[c];
    const int nch = (g.T + GAE_U - 1) / GAE_U;
    GaeChunk a, b;
    gae_load(g, c, e, g.T - 1, a);
    for (int k = 0; k < nch; k += 2) {
      const int ta = g.T - 1 - k * GAE_U, tb = ta - GAE_U;
      if (k + 1 < nch) gae_load(g, c, e, tb, b);
      gae_run(g, c, ta, a, acc, nextv, s1, s2);
      if (k + 1 >= nch) break;
      if (k + 2 < nch) gae_load(g, c, e, tb - GAE_U, a);
      gae_run(g, c, tb, b, acc, nextv, s1, s2);
    }
  }
  s1 = wave_sum_d(s1);
  s2 = wave_sum_d(s2);
  if (threadIdx.x == 0) {
    double* wp = g.partials + gae_wave_base(g.C) + 2 * blockIdx.x;
    wp[0] = s1;
    wp[1] = s2;
  }
