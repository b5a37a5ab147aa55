// Group finish: the kernels between a fragment's last env step and the update (gae.hip, episodes.hip)
// with a member axis.  M same-shaped contexts finish side by side: the member is blockIdx.z, chains,
// waves and envs are counted inside the member, and whatever differs between members (the record
// pointers, done flags, bootstrap values, GAE partials, adv_norm, the episode scratch, in-flight state
// and table) is read from a device table of FinishMember, indexed by the wave-uniform blockIdx.z.
//
// Equality contract: member m's outputs are, bit for bit, what the plain kernels write for that
// context alone.  It holds by construction: every kernel body is one text (gae_body.h,
// gae_finalize_body.h, ep_count_body.h, ep_scan_body.h, ep_walk_body.h) that the plain unit and this
// one include inside the kernel's braces, with the same chunk helpers (gae_chunk.h,
// episodes_chunk.h) and the same fp-contraction setting (off).  A kernel here is a signature and a
// prologue that builds the text's operand -- a local GaeArgs g or EpArgs a -- from the member's table
// entry and the by-value group arguments; the per-policy tables the walk indexes with a run-time
// policy are named by accessor macros, so they are read where they lie (kernel arguments, the table)
// and not from a local copy.
//
// What the texts rely on, for every member: the grids are the same for all members (sizes go by
// value), so the only early exits -- k_gae's past a policy's last wave, k_ep_count's past the last
// (t, w) -- are member-independent and whole waves reach the walk's ballots; the fp64 additions keep
// the texts' order; there is no atomic.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "gae_chunk.h"
#include "episodes_chunk.h"

namespace {
// the GaeArgs of policy p of member mb
__device__ __forceinline__ GaeArgs gae_member(const FinishGroupArgs& fa, const FinishMember& mb, int p) {
  GaeArgs g;
  g.rec = mb.rec[p]; g.lay = fa.lay[p]; g.C = fa.C[p]; g.T = fa.T; g.N = fa.N; g.k = fa.k[p];
  g.last_v = mb.last_v[p]; g.done_tn = mb.done_tn;
  g.gamma = fa.gamma; g.lambda_ = fa.lambda_;
  g.partials = mb.partials[p]; g.adv_norm = mb.adv_norm[p];
  return g;
}

// the EpArgs of member mb without the per-policy tables (EP_* accessors below)
__device__ __forceinline__ EpArgs ep_member(const FinishGroupArgs& fa, const FinishMember& mb) {
  EpArgs a{};
  a.N = fa.N; a.T = fa.T; a.n_agents = fa.n_agents; a.W = fa.W;
  a.done_tn = mb.done_tn; a.cnt = mb.ep_cnt; a.base = mb.ep_base; a.total = mb.ep_word;
  a.ep_total = mb.ep_total; a.ep_agent = mb.ep_agent; a.ep_len = mb.ep_len;
  a.table = mb.ep_table; a.cap = mb.ep_cap;
  return a;
}
}  // namespace

// ---- GAE: k_gae with grid (max_p ceil(C_p / 64), P, M), k_gae_finalize with grid (P, 1, M) ----
__global__ void __launch_bounds__(64) k_gae_group(FinishGroupArgs fa) {
  const GaeArgs g = gae_member(fa, fa.tab[blockIdx.z], blockIdx.y);
#include "gae_body.h"
}

__global__ void k_gae_finalize_group(FinishGroupArgs fa) {
  if (threadIdx.x != 0) return;
  const GaeArgs g = gae_member(fa, fa.tab[blockIdx.z], blockIdx.x);
#include "gae_finalize_body.h"
}

// ---- episode accounting: count (ceil(T W / 4), 1, M), scan (1, 1, M), walk (W, 1, M) ----
__global__ void __launch_bounds__(256) k_ep_count_group(FinishGroupArgs fa) {
  const EpArgs a = ep_member(fa, fa.tab[blockIdx.z]);
#include "ep_count_body.h"
}

// one workgroup per member; the member's total goes to its own word and to the group's totals[M],
// which the host reads in one copy
__global__ void __launch_bounds__(EP_SCAN_THREADS) k_ep_scan_group(FinishGroupArgs fa) {
  const EpArgs a = ep_member(fa, fa.tab[blockIdx.z]);
#define EP_SCAN_TOTAL(run) (a.total[0] = run, fa.totals[blockIdx.z] = run)
#include "ep_scan_body.h"
#undef EP_SCAN_TOTAL
}

__global__ void __launch_bounds__(64) k_ep_walk_group(FinishGroupArgs fa) {
  const FinishMember& mb = fa.tab[blockIdx.z];
  const EpArgs a = ep_member(fa, mb);
#define EP_POLICY_OF(j) fa.policy_of_agent[j]
#define EP_SLOT_OF(j) fa.slot_of_agent[j]
#define EP_K(p) fa.k[p]
#define EP_LAY(p) fa.lay[p]
#define EP_REC(p) mb.rec[p]
#include "ep_walk_body.h"
#undef EP_POLICY_OF
#undef EP_SLOT_OF
#undef EP_K
#undef EP_LAY
#undef EP_REC
}

void launch_finish_group_gae(hipStream_t s, const FinishGroupArgs& fa) {
  int maxw = 1;
  for (int p = 0; p < fa.P; ++p) maxw = maxw > (fa.C[p] + 63) / 64 ? maxw : (fa.C[p] + 63) / 64;
  hipLaunchKernelGGL(k_gae_group, dim3(maxw, fa.P, fa.M), dim3(64), 0, s, fa);
  hipLaunchKernelGGL(k_gae_finalize_group, dim3(fa.P, 1, fa.M), dim3(64), 0, s, fa);
}

void launch_finish_group_count_scan(hipStream_t s, const FinishGroupArgs& fa) {
  const int waves = fa.T * fa.W;
  hipLaunchKernelGGL(k_ep_count_group, dim3((waves + 3) / 4, 1, fa.M), dim3(256), 0, s, fa);
  hipLaunchKernelGGL(k_ep_scan_group, dim3(1, 1, fa.M), dim3(EP_SCAN_THREADS), 0, s, fa);
}

void launch_finish_group_walk(hipStream_t s, const FinishGroupArgs& fa) {
  hipLaunchKernelGGL(k_ep_walk_group, dim3(fa.W, 1, fa.M), dim3(64), 0, s, fa);
}
