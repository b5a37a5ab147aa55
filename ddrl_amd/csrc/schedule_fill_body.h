// The body of k_schedule_fill and k_schedule_fill_group (rng.hip), included inside the kernel's
// braces.  Operands by name: sm (the ScheduleMember: shuffle, perm, seed, draw), sh (the
// ScheduleShape).  Policy sh.pid[blockIdx.y]; lane i of its flat order shuffle | perm[0] | perm[1] ...
// computes its own element of the keyed bijection: no sort, no atomics, no other lane's value.
  const int p = sh.pid[blockIdx.y];
  const uint32_t R = (uint32_t)sh.R[p], nb = (uint32_t)sh.nb[p];
  const size_t total = (size_t)R + (size_t)sh.epochs * nb;
  const int h_R = philox::feistel_half_bits(R), h_nb = philox::feistel_half_bits(nb);
  int32_t* shuffle = sm.shuffle[p];
  int32_t* perm = sm.perm[p];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    if (i < R) {
      shuffle[i] = (int32_t)philox::feistel_permute(sm.seed, sm.draw, philox::schedule_tag(p, 0u), R, h_R, (uint32_t)i);
    } else {
      const size_t j = i - R;
      const uint32_t e = (uint32_t)(j / nb);
      perm[j] = (int32_t)philox::feistel_permute(sm.seed, sm.draw, philox::schedule_tag(p, 1u + e), nb, h_nb,
                                                 (uint32_t)(j - (size_t)e * nb));
    }
  }
