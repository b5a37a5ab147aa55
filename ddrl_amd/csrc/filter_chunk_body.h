// The body of k_filter_chunk (rollout.hip), k_filter_chunk_group (rollout_group.hip) and
// k_filter_chunk_members (eval_members.hip), included inside the kernel's braces.  Operands by name: obs [N][D], N, D, part (the chunk scratch).
  const int j = blockIdx.x, sc = blockIdx.y;
  __shared__ double red[4];
  const int tid = threadIdx.x, w = tid >> 6;
  const int e = sc * FP_ROWS + tid;
  const int n_c = min(FP_ROWS, N - sc * FP_ROWS);
  const float x = e < N ? obs[(size_t)e * D + j] : 0.f;
  double acc = wave_sum_d((double)x);
  if ((tid & 63) == 0) red[w] = acc;
  __syncthreads();
  const double mean_c = ((red[0] + red[1]) + (red[2] + red[3])) / (double)n_c;
  __syncthreads();
  const double dlt = e < N ? (double)x - mean_c : 0.0;
  acc = wave_sum_d(dlt * dlt);
  if ((tid & 63) == 0) red[w] = acc;
  __syncthreads();
  if (tid == 0) {
    double* pc = part + ((size_t)sc * D + j) * 2;
    pc[0] = mean_c;
    pc[1] = (red[0] + red[1]) + (red[2] + red[3]);
  }
