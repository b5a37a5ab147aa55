// The body of k_reward (rollout.hip) and k_reward_group (rollout_group.hip), included inside the
// kernel's braces.  Operands: ra (RewardArgs), fw, cfrc, actions, done_tn, and the unit's macros
// REWARD(field) for e0, rec and t (they differ between members) and REWARD_DONE(e), env e's done flag.
  const int na = ra.n_agents;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= ra.n * na) return;
  const int el = gid / na, j = gid - el * na, e = REWARD(e0) + el;
  const double r = agent_reward_d(ra, j, (double)fw[e], cfrc + (size_t)e * 14 * 6, actions + (size_t)e * 8);
  const int p = ra.policy_of_agent[j], slot = ra.slot_of_agent[j];
  const size_t C = (size_t)ra.N * ra.k[p];
  float* rp = REWARD(rec)[p] + ((size_t)REWARD(t) * C + (size_t)e * ra.k[p] + slot) * ra.lay[p].stride;
  rp[ra.lay[p].rew] = (float)r;
  if (j == 0) done_tn[(size_t)REWARD(t) * ra.N + e] = REWARD_DONE(e);
#undef REWARD
#undef REWARD_DONE
