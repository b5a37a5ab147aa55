// The text of k_ep_scan (episodes.hip) and k_ep_scan_group (finish_group.hip), included inside the
// kernel's braces.  Operands: a, the EpArgs (T, W, cnt, base are read), and EP_SCAN_TOTAL(run),
// the statement that stores the sum of the counts.
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
    EP_SCAN_TOTAL(run);
  }
  __syncthreads();
  long long run = part[threadIdx.x];
  for (int i = i0; i < i1; ++i) {
    a.base[i] = run;
    run += a.cnt[i];
  }
