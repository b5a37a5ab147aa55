// The body of k_filter_merge (rollout.hip), k_filter_merge_group (rollout_group.hip) and k_filter_merge_members
// (eval_members.hip), included inside the kernel's braces.  The counts are advanced by the kernel behind it.  Operands: N, D, part, the running (n_run, M, S) and delta (dn, dM, dS) stat, normc, push, enabled.
  const int j = threadIdx.x;
  if (j >= D) return;
  double n1 = n_run[0];
  double Mj = M[j], Sj = S[j];
  if (push) {
    // the batch's (mean, M2): the chunks merged in order (Chan et al.)
    const int nchunks = (N + FP_ROWS - 1) / FP_ROWS;
    double nb = 0.0, mean_b = 0.0, s_b = 0.0;
    for (int c = 0; c < nchunks; ++c) {
      const double* pc = part + ((size_t)c * D + j) * 2;
      const double nc = (double)min(FP_ROWS, N - c * FP_ROWS), nn = nb + nc, d = pc[0] - mean_b;
      mean_b = (nb * mean_b + nc * pc[0]) / nn;
      s_b = s_b + pc[1] + d * d * nb * nc / nn;
      nb = nn;
    }
    const double n2 = (double)N, n = n1 + n2;
    const double delta = Mj - mean_b;
    Mj = (n1 * Mj + n2 * mean_b) / n;
    Sj = Sj + s_b + delta * delta * n1 * n2 / n;
    n1 = n;
    M[j] = Mj;
    S[j] = Sj;
    // the same batch merged into the delta buffer (pushes since the last filter sync)
    const double d1 = dn[0], dd = d1 + n2, ddl = dM[j] - mean_b;
    dM[j] = (d1 * dM[j] + n2 * mean_b) / dd;
    dS[j] = dS[j] + s_b + ddl * ddl * d1 * n2 / dd;
  }
  const double var = n1 > 1.0 ? Sj / (n1 - 1.0) : Mj * Mj;
  normc[2 * j] = enabled ? Mj : 0.0;
  normc[2 * j + 1] = enabled ? sqrt(var) + 1e-8 : 1.0;
