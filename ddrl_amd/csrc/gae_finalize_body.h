// The text of k_gae_finalize (gae.hip) and k_gae_finalize_group (finish_group.hip), included inside
// the kernel's braces behind `if (threadIdx.x != 0) return;`.  Operand: g, the GaeArgs of this
// block's policy (blockIdx.x).
  const int nw = (g.C + 63) / 64, ngroups = (g.C + 255) / 256;
  const double* wp = g.partials + gae_wave_base(g.C);
  double s1 = 0.0, s2 = 0.0;
  for (int b = 0; b < ngroups; ++b) {
    double x[2][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int w = 4 * b + i;
      x[0][i] = w < nw ? wp[2 * w] : 0.0;
      x[1][i] = w < nw ? wp[2 * w + 1] : 0.0;
    }
    s1 += (x[0][0] + x[0][1]) + (x[0][2] + x[0][3]);
    s2 += (x[1][0] + x[1][1]) + (x[1][2] + x[1][3]);
  }
  const double n = (double)g.C * (double)g.T;
  double* tot = g.partials + 2 * ngroups;   // for a cross-rank StandardizeFields
  tot[0] = s1;
  tot[1] = s2;
  tot[2] = n;
  const double mean = s1 / n;
  double var = s2 / n - mean * mean;
  if (var < 0.0) var = 0.0;
  const float std32 = (float)sqrt(var);
  g.adv_norm[0] = (float)mean;
  g.adv_norm[1] = fmaxf(1e-4f, std32);
