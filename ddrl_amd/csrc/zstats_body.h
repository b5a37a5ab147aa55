// The body of k_zstats (rollout.hip) and k_zstats_group (rollout_group.hip), included inside the
// kernel's braces.  Operands by name: obs [N][D], N, D, normc, clip, zs.
  const int j = blockIdx.x, tid = threadIdx.x;
  __shared__ double red[2][4];
  double s1 = 0.0, s2 = 0.0;
  for (int e = tid; e < N; e += 256) {
    const double z = norm_obs_d(obs[(size_t)e * D + j], normc, j, clip);
    s1 += z;
    s2 += z * z;
  }
  s1 = wave_sum_d(s1);
  s2 = wave_sum_d(s2);
  if ((tid & 63) == 0) { red[0][tid >> 6] = s1; red[1][tid >> 6] = s2; }
  __syncthreads();
  if (tid == 0) {
    zs[2 * j] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    zs[2 * j + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
