// The body of k_observe_ffn (rollout.hip) and k_observe_ffn_group (rollout_group.hip), included inside the
// kernel's braces.  Operands: ra (RouteArgs), obs, normc, clip, stage_tab, pf, and the unit's OBSERVE_E0 (first env).
  const int p = blockIdx.y;
  const PolicyRoute& pr = ra.pol[p];
  const int C = ra.N * pr.k;              // rows of the env range [e0, e0 + N)
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= C * pr.d) return;
  const int cl = gid / pr.d, f = gid - cl * pr.d;
  const int el = cl / pr.k, slot = cl - el * pr.k;
  const int e = OBSERVE_E0 + el, c = OBSERVE_E0 * pr.k + cl;
  stage_tab[p][(size_t)c * pr.d + f] =
      routed_input(pr, slot, f, obs + (size_t)e * ra.full_dim, normc, clip, policy_filter_normc(pf, p));
#undef OBSERVE_E0
