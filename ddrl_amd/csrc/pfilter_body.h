// The body of k_pfilter (rollout.hip) and k_pfilter_group (rollout_group.hip), included inside the
// kernel's braces.  Operands by name: ra (RouteArgs), zs, pf, update.
  const int p = blockIdx.x, f = threadIdx.x;
  const PolicyRoute& pr = ra.pol[p];
  double* P = pf + (size_t)p * PF_STRIDE;
  const double n0 = P[PF_N], dn0 = P[PF_DN];
  const double nb = (double)ra.N * pr.k;
  __syncthreads();
  if (f < pr.d) {
    double M = P[PF_M + f], S = P[PF_S + f], n = n0;
    if (update) {
      double s1 = 0.0, s2 = 0.0;
      for (int s = 0; s < pr.k; ++s) {
        const int idx = pr.obs_index[s][f];
        s1 += zs[2 * idx];
        s2 += zs[2 * idx + 1];
      }
      const double mb = s1 / nb, sb = fmax(s2 - s1 * mb, 0.0);
      chan_merge(n, M, S, nb, mb, sb);
      double dn = dn0, dM = P[PF_DM + f], dS = P[PF_DS + f];
      chan_merge(dn, dM, dS, nb, mb, sb);
      P[PF_M + f] = M;
      P[PF_S + f] = S;
      P[PF_DM + f] = dM;
      P[PF_DS + f] = dS;
      n = n0 + nb;
    }
    const double var = n > 1.0 ? S / (n - 1.0) : M * M;
    P[PF_NORMC + 2 * f] = M;
    P[PF_NORMC + 2 * f + 1] = sqrt(var) + 1e-8;
  }
  __syncthreads();
  if (update && f == 0) {
    P[PF_N] = n0 + nb;
    P[PF_DN] = dn0 + nb;
  }
