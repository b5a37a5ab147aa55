// Episode accounting of the training rollout: the returns and lengths of the episodes that
// finish in a fragment, as RLlib 1.0 counts them.
//
// RLlib MultiAgentEpisode._add_agent_rewards: for every env step, for every agent in agent order,
//   agent_rewards[(agent, policy)] += r;  total_reward += r      (Python floats: fp64),
// length counts env steps, and the step that raises done belongs to the episode it ends.  The
// total is an interleaved sum, not the sum of the per-agent totals.  An episode spans several
// fragments, so the running sums of every env stay in the context between calls.
//
// The reward added is the fp32 `rew` field of the agent's record (what the learner trains on),
// widened to fp64.  Agent j of env e is row c = e * k_p + slot of policy p = policy_of_agent[j],
// the mapping k_reward writes with.
//
// Output: one row of 8 doubles (a 64-byte line) per finished episode,
//   {t, env, length, total, agent_0 .. agent_3}   (agents the env does not have: NaN),
// in ascending (t, env) order.  The row position is counts + an exclusive scan + the rank of the
// lane in its wave's ballot: nothing depends on timing, and there is no atomic of any kind.
//   k_ep_count: cnt[t][w] = popcount of the ballot of done_tn[t][64 w .. 64 w + 63];
//   k_ep_scan:  base = exclusive scan of cnt in (t, w) order (one workgroup), total to a word;
//   k_ep_walk:  one thread per env, one wave per 64 consecutive envs, forward over t.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "episodes_chunk.h"

// The kernel bodies are texts of their own (ep_count_body.h, ep_scan_body.h, ep_walk_body.h; the
// chunk helpers in episodes_chunk.h), included inside the braces here and in finish_group.hip,
// which runs them with a member axis.
__global__ void __launch_bounds__(256) k_ep_count(EpArgs a) {
#include "ep_count_body.h"
}

// Exclusive scan of n = T * W counts by one workgroup: every thread sums a contiguous run,
// thread 0 scans the 256 run totals, every thread writes its run's bases.
__global__ void __launch_bounds__(EP_SCAN_THREADS) k_ep_scan(EpArgs a) {
#define EP_SCAN_TOTAL(run) a.total[0] = run
#include "ep_scan_body.h"
#undef EP_SCAN_TOTAL
}

__global__ void __launch_bounds__(64) k_ep_walk(EpArgs a) {
#define EP_POLICY_OF(j) a.policy_of_agent[j]
#define EP_SLOT_OF(j) a.slot_of_agent[j]
#define EP_K(p) a.k[p]
#define EP_LAY(p) a.lay[p]
#define EP_REC(p) a.rec[p]
#include "ep_walk_body.h"
#undef EP_POLICY_OF
#undef EP_SLOT_OF
#undef EP_K
#undef EP_LAY
#undef EP_REC
}

void launch_ep_count_scan(hipStream_t s, const EpArgs& a) {
  const int waves = a.T * a.W;
  hipLaunchKernelGGL(k_ep_count, dim3((waves + 3) / 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_ep_scan, dim3(1), dim3(EP_SCAN_THREADS), 0, s, a);
}

void launch_ep_walk(hipStream_t s, const EpArgs& a) {
  hipLaunchKernelGGL(k_ep_walk, dim3(a.W), dim3(64), 0, s, a);
}
