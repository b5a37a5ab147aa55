// The row pipeline around the fcnet forward, shared by the rollout kernels (rollout.hip and, through
// the same body texts, rollout_group.hip), the fused evaluation forward (eval.hip, eval_members.hip)
// and the input-sensitivity kernel (eval_sens.hip): the
// observation arithmetic (env-side normalization, routing, per-policy filter), the action
// epilogue (clip, sign flip, scatter) and the per-agent reward.  One body each,
// so the kernels agree bit for bit by construction; every function is force-inlined into its
// caller and compiled with the fp-contraction setting of the caller's translation unit (this
// header sets none).
//
// Reference: simulation_envs/quantruped_adaptor_multi_environment.py:83-85 (normalize),
// :124-136 (distribute_observations), :160-212 (contact cost, rewards, concatenate_actions);
// RLlib MeanStdFilter (get_filter, clip=None) and clip_actions=True.
#pragma once
#include "common.h"
#include "kernels.h"

// ---- observations --------------------------------------------------------------------
// The running count of the env-side filter advances after every column of k_filter_merge has
// read it: the kernel that follows adds the batch (FilterCount: count = N, or 0 when the
// filter did not push).
__device__ __forceinline__ void filter_count(const FilterCount& fc) {
  if (fc.count && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    fc.n_run[0] += (double)fc.count;
    fc.dn[0] += (double)fc.count;
  }
}

// env-side MeanStdFilter: (x - mean) / (std + 1e-8) in fp64, clipped when clip > 0
__device__ __forceinline__ double norm_obs_d(float x, const double* normc, int idx, float clip) {
  double z = ((double)x - normc[2 * idx]) / normc[2 * idx + 1];
  if (clip > 0.f) z = fmin(fmax(z, -(double)clip), (double)clip);
  return z;
}
__device__ __forceinline__ float norm_obs(float x, const double* normc, int idx, float clip) {
  return (float)norm_obs_d(x, normc, idx, clip);
}

// RunningStat.update (Chan et al.): the batch (nb, mb, sb) merged into the running (n, M, S), n left to the caller
__device__ __forceinline__ void chan_merge(double& n, double& M, double& S, double nb, double mb, double sb) {
  const double tot = n + nb, delta = M - mb;
  M = (n * M + nb * mb) / tot;
  S = S + sb + delta * delta * n * nb / tot;
}

// the normalization constants (mean, std + 1e-8 per column) of policy p's filter; null: no filter
__device__ __forceinline__ const double* policy_filter_normc(const double* pf, int p) {
  return pf ? pf + (size_t)p * PF_STRIDE + PF_NORMC : nullptr;
}

// Input f of a (slot) row, in two levels.  First: obs_index[slot][f] names a column of the env's
// raw observation (norm_obs_d gives its env-normalized fp64 value) or, below zero, is the code
// of a constant input (-1: 0, -2: 1), which nothing filters or perturbs.
__device__ __forceinline__ float const_input(int idx) { return idx == -2 ? 1.f : 0.f; }
// Second: the policy's fp32 input from a routed value.  P (policy_filter_normc): the RLlib
// MeanStdFilter runs on the fp64 env-normalized value.
__device__ __forceinline__ float policy_input(double z, const double* P, int f) {
  if (P) return (float)((z - P[2 * f]) / P[2 * f + 1]);
  return (float)z;
}
// Both levels in one, for the kernels that put nothing between them (k_eval_sens adds its step
// between the two).  The filter test comes before the normalization on purpose: with the
// normalization first the compiler shares it and pays one more divergent region per operand,
// which k_eval_act has on its critical path (measured: + 0.35 us per launch).
__device__ __forceinline__ float routed_input(const PolicyRoute& pr, int slot, int f, const float* o,
                                              const double* normc, float clip, const double* P) {
  const int idx = pr.obs_index[slot][f];
  if (idx < 0) return const_input(idx);
  if (P) return policy_input(norm_obs_d(o[idx], normc, idx, clip), P, f);
  return norm_obs(o[idx], normc, idx, clip);
}

// ---- actions -------------------------------------------------------------------------
__device__ __forceinline__ float clip_action(float a) { return fminf(fmaxf(a, -1.f), 1.f); }
// component j of the slot's action as the env takes it: clipped, then LegTransforms' sign
__device__ __forceinline__ float env_action(const PolicyRoute& pr, int slot, int j, float a) {
  const float ac = clip_action(a);
  return (pr.act_neg[slot] >> j) & 1 ? -ac : ac;
}
__device__ __forceinline__ void scatter_action(float* actions, const PolicyRoute& pr, int e, int slot, int j,
                                               float a) {
  actions[(size_t)e * 8 + pr.act_index[slot][j]] = env_action(pr, slot, j, a);
}

// ---- reward (a8) ---------------------------------------------------------------------
// Agent j's reward of a step, fp64 like the reference: per-leg (mode 0), global (1) or
// normalized (2); cf = the env's contact forces [14][6], a8 = its action vector.
__device__ __forceinline__ double agent_reward_d(const RewardArgs& ra, int j, double fwd, const float* cf,
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
