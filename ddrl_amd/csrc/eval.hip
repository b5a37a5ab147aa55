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

// The observation arithmetic of rollout.hip's observe kernels, restated so that the training
// kernels' translation unit stays as it is: env-side normc with clip in fp64, the running
// count of a push added by one thread after k_filter_merge has read it.
__device__ __forceinline__ void eval_filter_count(const FilterCount& fc) {
  if (fc.count && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    fc.n_run[0] += (double)fc.count;
    fc.dn[0] += (double)fc.count;
  }
}
__device__ __forceinline__ double eval_norm_obs_d(float x, const double* normc, int idx, float clip) {
  double z = ((double)x - normc[2 * idx]) / normc[2 * idx + 1];
  if (clip > 0.f) z = fmin(fmax(z, -(double)clip), (double)clip);
  return z;
}
__device__ __forceinline__ float eval_norm_obs(float x, const double* normc, int idx, float clip) {
  double z = ((double)x - normc[2 * idx]) / normc[2 * idx + 1];
  if (clip > 0.f) z = fmin(fmax(z, -(double)clip), (double)clip);
  return (float)z;
}

// ------------------------------------------------------------------------------------
// Fused evaluation forward.  Workgroup = 4 waves = 64 rows of ONE policy (grid.y = policy),
// the policy branch's weights staged into LDS in k_act_ffn's image; wave w runs the policy
// branch of row tile w.  Every lane builds its layer-1 operands X[row = c][f = 4 s + q] straight from
// the raw observation (k_observe_ffn's expression: env-side normalization, the per-policy
// filter's constants, the obs_index gather with the -1 / -2 constants), so nothing is staged
// in HBM.  Action = mean (eps == nullptr) or mean + exp(log_std) * eps, clipped, sign-flipped
// and scattered into the env action vector.  No value branch, no record.
// ------------------------------------------------------------------------------------
// The policy branch's half of stage_weights' LDS image (ffn.h): the same swizzled w1 / w2 and
// the same b1 / b2 / wo / bo, without the value branch this kernel never runs.
#define LDS_POLICY_FLOATS(O) (LDS_W1 + LDS_W2 + 2 * 64 + 64 * (O) + (O))
__device__ __forceinline__ void stage_policy_weights(const float* __restrict__ th, int d, int A, float* lds,
                                                     NetLds& P, int nthreads) {
  const FfnOffsets o = ffn_offsets(d, A);
  const int O = 2 * A;
  P.w1 = lds;         P.w2 = P.w1 + LDS_W1;
  P.b1 = P.w2 + LDS_W2;  P.b2 = P.b1 + 64;
  P.wo = P.b2 + 64;   P.bo = P.wo + 64 * O;
  const int tid = threadIdx.x;
  for (int i = tid; i < 48 * 64; i += nthreads) {
    const int f = i >> 6, col = i & 63;
    P.w1[sidx(f, col)] = f < d ? th[o.w1 + i] : 0.f;
  }
  for (int i = tid; i < 64 * 64; i += nthreads) P.w2[sidx(i >> 6, i & 63)] = th[o.w2 + i];
  for (int i = tid; i < 64; i += nthreads) {
    P.b1[i] = th[o.b1 + i];
    P.b2[i] = th[o.b2 + i];
  }
  for (int i = tid; i < 64 * O; i += nthreads) P.wo[i] = th[o.wo + i];
  for (int i = tid; i < O; i += nthreads) P.bo[i] = th[o.bo + i];
}

template <int A, int KS1>
__global__ void __launch_bounds__(256) k_eval_act(RouteArgs ra, EvalActArgs ea) {
  constexpr int O = 2 * A;
  extern __shared__ float lds[];
  eval_filter_count(ea.fc);
  const int p = blockIdx.y;
  const PolicyRoute& pr = ra.pol[p];
  const int row_hi = ra.N * pr.k;
  const int row0 = blockIdx.x * 64;
  if (row0 >= row_hi) return;
  const int d = pr.d;
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4, w = threadIdx.x >> 6;
  const int row = row0 + 16 * w + c;
  const bool valid = row < row_hi;
  const int rv = valid ? row : 0;
  const int e = rv / pr.k, slot = rv - e * pr.k;
  const float* o = ea.obs + (size_t)e * ra.full_dim;
  const double* P = ea.pf ? ea.pf + (size_t)p * PF_STRIDE + PF_NORMC : nullptr;
  float xop[12];
#pragma unroll
  for (int s = 0; s < 12; ++s) {
    const int f = 4 * s + q;
    float v = 0.f;
    if (s < KS1 && f < d && valid) {
      const int idx = pr.obs_index[slot][f];
      if (idx < 0) {
        v = idx == -2 ? 1.f : 0.f;
      } else if (P) {   // RLlib MeanStdFilter on the fp64 env-normalized value
        v = (float)((eval_norm_obs_d(o[idx], ea.normc, idx, ea.clip) - P[2 * f]) / P[2 * f + 1]);
      } else {
        v = eval_norm_obs(o[idx], ea.normc, idx, ea.clip);
      }
    }
    xop[s] = v;
  }
  // the weights are staged after the operand loads were issued: the fp64 normalization runs
  // while the weight loads are in flight
  NetLds PW;
  stage_policy_weights(ea.theta[p], d, A, lds, PW, 256);
  __syncthreads();
  floatx4 h1[4], h2[4];
  float logits[O];
  ffn_branch_fwd<O, KS1>(PW, xop, h1, h2, logits);
  if (!valid) return;
  const int agent = pr.agent[slot];
  // "cup" model: mean_j *= coupling[leg][j], leg = the agent's slot (k_act_ffn)
  if (ea.cup[p]) {
#pragma unroll
    for (int j = 0; j < A; ++j) logits[j] *= ea.cup[p][slot * A + j];
  }
  if (q == 0) {
#pragma unroll
    for (int j = 0; j < A; ++j) {
      const float mu = logits[j], ls = logits[A + j];
      float act = mu;   // deterministic: the DiagGaussian mean (explore=False)
      if (ea.eps) {
        const float sd = expf(ls);
        const float eps = ea.eps[((size_t)e * ra.n_agents + agent) * A + j];
        act = mu + sd * eps;
      }
      const float ac = fminf(fmaxf(act, -1.f), 1.f);
      ea.actions[(size_t)e * 8 + pr.act_index[slot][j]] = (pr.act_neg[slot] >> j) & 1 ? -ac : ac;
    }
  } else if (q == 1 && ea.logits_out[p]) {
    float* lo = ea.logits_out[p] + (size_t)row * O;
#pragma unroll
    for (int j = 0; j < O; ++j) lo[j] = logits[j];
  }
}

template <int A, int KS1>
static void launch_eval_act_t(hipStream_t s, dim3 grid, const RouteArgs& ra, const EvalActArgs& ea) {
  hipLaunchKernelGGL((k_eval_act<A, KS1>), grid, dim3(256), LDS_POLICY_FLOATS(2 * A) * 4, s, ra, ea);
}

void launch_eval_act(hipStream_t s, const RouteArgs& ra, const EvalActArgs& ea) {
  int maxC = 0, maxd = 0;
  for (int p = 0; p < ra.P; ++p) {
    maxC = max(maxC, ra.N * ra.pol[p].k);
    maxd = max(maxd, ra.pol[p].d);
  }
  dim3 grid((maxC + 63) / 64, ra.P);
  DDRL_DISPATCH_A_KS1(ra.A, maxd, launch_eval_act_t, s, grid, ra, ea);
}

// ------------------------------------------------------------------------------------
// Episode statistics, all fp64 (the reference sums Python floats).  Four lanes per env: lane j
// computes agent j's reward of the step (k_reward's formula, restated, not rounded to fp32),
// lane 0 adds them in agent order (rollout_episodes.py:122 sum(reward.values())) and keeps the
// env's accumulators: return, power += sum_j |ctrl[(j + roll) & 7] * qvel[j]| (:146),
// distance += dx, steps += 1.  On done the env writes row (e, ep_count[e]) = {return, steps,
// distance, power, velocity, CoT} (:149-151) while it is below its quota of E episodes, and
// restarts its accumulators either way.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ double eval_agent_reward(const RewardArgs& ra, int j, double fwd, const float* cf,
                                                    const float* a8) {
  const int na = ra.n_agents;
  if (ra.mode == 1) {
    double ctrl_all = 0.0, contact_all = 0.0;
    for (int i = 0; i < 8; ++i) ctrl_all += (double)a8[i] * a8[i];
    for (int i = 0; i < 14 * 6; ++i) {
      const double v = fmin(fmax((double)cf[i], -1.0), 1.0);
      contact_all += v * v;
    }
    contact_all *= ra.contact_w;
    return (fwd - ra.ctrl_w * ctrl_all - contact_all) / na;
  }
  double ctrl = 0.0;
  for (int i = 0; i < ra.n_act[j]; ++i) {
    const double a = a8[ra.act_index[j][i]];
    ctrl += a * a;
  }
  double contact = 0.0;
  for (int b = 0; b < ra.n_contact[j]; ++b) {
    const float* body = cf + ra.contact_index[j][b] * 6;
    double sb = 0.0;
    for (int k = 0; k < 6; ++k) {
      const double v = fmin(fmax((double)body[k], -1.0), 1.0);
      sb += ra.contact_w * v * v * ra.contact_weight[j][b];
    }
    contact += sb;
  }
  return ra.mode == 2 ? fwd - na * (ra.ctrl_w * ctrl + contact) : fwd / na - ra.ctrl_w * ctrl - contact;
}

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
  const double r = j < ra.n_agents ? eval_agent_reward(ra, j, (double)fw[e], cfrc + (size_t)e * 14 * 6, a8) : 0.0;
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
