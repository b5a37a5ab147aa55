// Evaluation-side kernels: the fused per-step policy forward of a trained policy (observe +
// route + forward + action in one launch, no training record) and the per-env episode
// statistics the reference's evaluation reports.
//
// Reference: evaluation/rollout_episodes.py:26-164 (episode loop, reward / power / distance
// accumulation, velocity and cost of transport), driven by
// evaluation/evaluate_trained_policies_pd.py:84-127; RLlib compute_action (filters with
// update=False; explore=False takes the DiagGaussian mean).
#include "common.h"
#include "kernels.h"
#include "ffn.h"
#include "policy_io.h"

// ------------------------------------------------------------------------------------
// Fused evaluation forward.  Workgroup = 4 waves = 64 rows of ONE policy (grid.y = policy),
// the policy branch's weights staged into LDS in k_act_ffn's image; wave w runs the policy
// branch of row tile w.  Every lane builds its layer-1 operands X[row = c][f = 4 s + q] straight from
// the raw observation (policy_io.h: the expression k_observe_ffn stages), so nothing is staged
// in HBM.  Action = mean (eps == nullptr) or mean + exp(log_std) * eps, clipped, sign-flipped
// and scattered into the env action vector.  No value branch, no record.
// ------------------------------------------------------------------------------------
template <int A, int KS1>
__global__ void __launch_bounds__(256) k_eval_act(RouteArgs ra, EvalActArgs ea) {
  filter_count(ea.fc);
  // eval_<field>: where the plain arguments keep that operand; policy p's are macros (p is the text's)
  const auto &eval_obs = ea.in.obs, &eval_eps = ea.eps;
  const auto &eval_normc = ea.in.normc, &eval_pf = ea.in.pf;
  const auto& eval_clip = ea.in.clip;
  const auto& eval_actions = ea.actions;
#define eval_theta ea.in.theta[p]
#define eval_cup ea.in.cup[p]
#define eval_logits_out ea.logits_out[p]
#define EVAL(field) eval_##field
#define EVAL_TILE_GUARD
#include "eval_act_body.h"
#undef eval_theta
#undef eval_cup
#undef eval_logits_out
}

template <int A, int KS1>
static void launch_eval_act_t(hipStream_t s, dim3 grid, const RouteArgs& ra, const EvalActArgs& ea) {
  hipLaunchKernelGGL((k_eval_act<A, KS1>), grid, dim3(256), LDS_POLICY_FLOATS(2 * A) * 4, s, ra, ea);
}

void launch_eval_act(hipStream_t s, const RouteArgs& ra, const EvalActArgs& ea) {
  const RowGeom g = row_geom(ra, ra.N);
  dim3 grid((g.rows + 63) / 64, ra.P);
  DDRL_DISPATCH_A_KS1(ra.A, g.d, launch_eval_act_t, s, grid, ra, ea);
}

// ------------------------------------------------------------------------------------
// Episode statistics, all fp64 (the reference sums Python floats).  Four lanes per env: lane j
// computes agent j's reward of the step (agent_reward_d, k_reward's; not rounded to fp32),
// lane 0 adds them in agent order (rollout_episodes.py:122 sum(reward.values())) and keeps the
// env's accumulators: return, power += sum_j |ctrl[(j + roll) & 7] * qvel[j]| (:146),
// distance += dx, steps += 1.  On done the env writes row (e, ep_count[e]) = {return, steps,
// distance, power, velocity, CoT} (:149-151) while it is below its quota of E episodes, and
// restarts its accumulators either way.
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_eval_accum(RewardArgs ra, EvalAccumArgs ev,
                                                    const float* __restrict__ fw,
                                                    const float* __restrict__ cfrc,
                                                    const float* __restrict__ actions,
                                                    const float* __restrict__ kin,
                                                    const uint8_t* __restrict__ done) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int el = gid >> 2, j = gid & 3;
  const int e = min(el, ra.N - 1);   // lanes past the last env compute on it and write nothing
  const float* a8 = actions + (size_t)e * 8;
  const double r = j < ra.n_agents ? agent_reward_d(ra, j, (double)fw[e], cfrc + (size_t)e * 14 * 6, a8) : 0.0;
  // every lane of the wave takes part in the exchange; agents are added in order
  const int base = (threadIdx.x & 63) & ~3;
  double step_reward = __shfl(r, base);
  for (int a = 1; a < DDRL_MAXAG; ++a) {
    const double other = __shfl(r, base + a);
    if (a < ra.n_agents) step_reward += other;
  }
  if (j != 0 || el >= ra.N) return;
  const float* kn = kin + (size_t)e * 9;
  double* acc = ev.acc + (size_t)e * 4;   // return, power, distance, steps
  const double ret = acc[0] + step_reward;
  // np.sum of 8 doubles: numpy's unrolled pairwise order
  double pw[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) pw[i] = fabs((double)a8[(i + ev.ctrl_roll) & 7] * (double)kn[1 + i]);
  const double power = acc[1] + (((pw[0] + pw[1]) + (pw[2] + pw[3])) + ((pw[4] + pw[5]) + (pw[6] + pw[7])));
  const double dist = acc[2] + (double)kn[0];
  const double steps = acc[3] + 1.0;
  if (!done[e]) {
    acc[0] = ret; acc[1] = power; acc[2] = dist; acc[3] = steps;
    return;
  }
  const int cnt = ev.ep_count[e];
  if (cnt < ev.E) {
    double* row = ev.table + ((size_t)e * ev.E + cnt) * 6;
    const double vel = dist / steps;
    row[0] = ret; row[1] = steps; row[2] = dist; row[3] = power; row[4] = vel;
    row[5] = (power / steps) / (ev.total_mass * vel);
    ev.ep_count[e] = cnt + 1;
    atomicAdd(&ev.counters[0], 1ull);                       // episodes recorded
    if (cnt + 1 == ev.E) atomicAdd(&ev.counters[1], 1ull);  // envs that filled their quota
  }
  acc[0] = 0.0; acc[1] = 0.0; acc[2] = 0.0; acc[3] = 0.0;
}

void launch_eval_accum(hipStream_t s, const RewardArgs& ra, const EvalAccumArgs& ev, const float* fw,
                       const float* cfrc, const float* actions, const float* kin, const uint8_t* done) {
  hipLaunchKernelGGL(k_eval_accum, dim3((4 * ra.N + 255) / 256), dim3(256), 0, s, ra, ev, fw, cfrc, actions, kin,
                     done);
}
