// The text of k_ep_count (episodes.hip) and k_ep_count_group (finish_group.hip), included inside
// the kernel's braces.  Operand: a, the EpArgs (N, T, W, done_tn, cnt are read).
  const int gw = (blockIdx.x * 256 + threadIdx.x) >> 6;   // wave = (t, w)
  const int lane = threadIdx.x & 63;
  if (gw >= a.T * a.W) return;                             // whole waves leave together
  const int t = gw / a.W, w = gw - t * a.W;
  const int e = w * 64 + lane;
  const bool d = e < a.N && a.done_tn[(size_t)t * a.N + e] != 0;
  const unsigned long long m = __ballot(d);
  if (lane == 0) a.cnt[gw] = __popcll(m);
