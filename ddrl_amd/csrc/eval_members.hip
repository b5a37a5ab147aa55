// Evaluation members: M parameter sets evaluated side by side on one context, n envs each (the
// reference's sweeps -- evaluation/evaluate_trained_policies_pd.py:84-127 and
// evaluate_trained_policies_tvel_range_pd.py:52-78 roll out one restored agent per cell).  Member
// m owns the envs [m n, (m + 1) n); its weights, env-side filter and per-policy filter constants
// live at base + m * stride (kernels.h EvalMembersArgs).
//
// Equality contract: a member computes, bit for bit, what a plain context of n envs holding its
// state computes.  It holds by construction, as in rollout_group.hip: every kernel body is one text
// (*_body.h) that the plain unit (eval.hip, rollout.hip) and this one include inside the kernel's
// braces.  A kernel here is a signature and a prologue that names the text's operands at the
// member's own bases, so the text counts envs, rows and filter chunks inside the member.
#include "common.h"
#include "kernels.h"
#include "ffn.h"
#include "policy_io.h"

// ---- k_eval_act with grid (ceil(n k_max / 64), P, M) ----
// The count of the pushed batch is added here, by one thread of the member's first block: after
// the member's merge kernel (the only reader of the old count) and once per member.  A wave whose
// 16-row tile lies past the member's last row helps to stage the weights, meets the barrier and
// leaves before the MFMAs.
template <int A, int KS1>
__global__ void __launch_bounds__(256) k_eval_act_members(RouteArgs ra, EvalMembersArgs ma, int count) {
  const size_t m = blockIdx.z;
  double* F = ma.filt + m * FM_STRIDE;
  filter_count(FilterCount{F + FM_N, F + FM_DN, count});
  // eval_<field>: the member's base of that operand.  Macros, formed where the text reads them (p, row_hi and O
  // are the text's): as locals their scalar loads and null tests line up ahead of the first row's work
  const double* eval_normc = F + FM_NORMC;
  const auto& eval_clip = ma.clip;
#define eval_obs (ma.obs + m * ra.N * ra.full_dim)
#define eval_pf (ma.pf ? ma.pf + m * ma.pf_stride : nullptr)
#define eval_theta (ma.theta[p] + m * ma.theta_stride[p])
#define eval_cup (ma.cup_off[p] >= 0 ? eval_theta + ma.cup_off[p] : nullptr)
#define eval_eps (ma.eps ? ma.eps + m * ra.N * ra.n_agents * A : nullptr)
#define eval_actions (ma.actions + m * ra.N * 8)
#define eval_logits_out (ma.logits_out[p] ? ma.logits_out[p] + m * row_hi * O : nullptr)
#define EVAL(field) eval_##field
#define EVAL_TILE_GUARD if (row0 + 16 * w >= row_hi) return;   // wave-uniform: an empty tile, and no barrier follows
#include "eval_act_body.h"
#undef eval_obs
#undef eval_pf
#undef eval_theta
#undef eval_cup
#undef eval_eps
#undef eval_actions
#undef eval_logits_out
}

template <int A, int KS1>
static void launch_eval_act_members_t(hipStream_t s, dim3 grid, const RouteArgs& ra, const EvalMembersArgs& ma,
                                      int count) {
  hipLaunchKernelGGL((k_eval_act_members<A, KS1>), grid, dim3(256), LDS_POLICY_FLOATS(2 * A) * 4, s, ra, ma, count);
}

void launch_eval_act_members(hipStream_t s, const RouteArgs& ra, const EvalMembersArgs& ma, int n_members, int count) {
  const RowGeom g = row_geom(ra, ra.N);
  dim3 grid((g.rows + 63) / 64, ra.P, n_members);
  DDRL_DISPATCH_A_KS1(ra.A, g.d, launch_eval_act_members_t, s, grid, ra, ma, count);
}

// ---- env-side filter push: k_filter_chunk / k_filter_merge, chunks counted from the member's first env ----
__global__ void __launch_bounds__(256) k_filter_chunk_members(const float* __restrict__ obs_all, int N, int D,
                                                              double* __restrict__ part_all, size_t part_stride) {
  const float* obs = obs_all + (size_t)blockIdx.z * N * D;
  double* part = part_all + blockIdx.z * part_stride;
#include "filter_chunk_body.h"
}

__global__ void __launch_bounds__(64) k_filter_merge_members(int N, int D, const double* __restrict__ part_all,
                                                             size_t part_stride, double* filt, int push, int enabled) {
  const double* part = part_all + blockIdx.z * part_stride;
  double* F = filt + (size_t)blockIdx.z * FM_STRIDE;
  double *n_run = F + FM_N, *M = F + FM_M, *S = F + FM_S, *normc = F + FM_NORMC;
  double *dn = F + FM_DN, *dM = F + FM_DM, *dS = F + FM_DS;
#include "filter_merge_body.h"
}

void launch_filter_push_members(hipStream_t s, const float* obs, int n, int D, int n_members, double* filt,
                                int update, int enabled, double* part) {
  const int push = enabled && update;
  const size_t part_stride = filter_part_doubles(n, D);
  if (push)
    hipLaunchKernelGGL(k_filter_chunk_members, dim3(D, (n + FP_ROWS - 1) / FP_ROWS, n_members), dim3(256), 0, s, obs,
                       n, D, part, part_stride);
  hipLaunchKernelGGL(k_filter_merge_members, dim3(1, 1, n_members), dim3(64), 0, s, n, D, part, part_stride, filt,
                     push, enabled);
}
