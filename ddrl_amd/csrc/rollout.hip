// Rollout-side kernels: env-side MeanStdFilter (a2), observation routing (a1/a3),
// fused per-policy forward + DiagGaussian sampling + action scatter (a4/a6/a7),
// per-leg rewards (a8).
//
// Reference: simulation_envs/quantruped_adaptor_multi_environment.py:83-85 (normalize),
// :124-136 (distribute_observations), :160-212 (contact cost, rewards, concatenate_actions);
// models/fcnet_glorot_uniform_init.py:120-125 (forward / value_function);
// RLlib DiagGaussian sampling with clip_actions=True.
//
// The bodies of the kernels of a device-plane training step (filter chunk / merge, zstats / pfilter,
// observe, act, reward) are texts of their own (*_body.h), included inside the kernel's braces here and
// in rollout_group.hip's member-axis kernels: the signature names the operands, an accessor macro the
// fields of a by-value argument block the text reads (defined here, undefined at the text's end).
#include "common.h"
#include "kernels.h"
#include "ffn.h"
#include "policy_io.h"

// ------------------------------------------------------------------------------------
// a2: batched MeanStdFilter push, two launches.  k_filter_chunk: workgroup (j, s) reduces rows
// [256 s, 256 s + 256) of observation column j to the chunk's (mean, M2) in fp64 (two passes
// over one value per thread, fixed-order wave / workgroup sums).  k_filter_merge: one thread
// per column merges the chunks in order with Chan's formula into the batch's (mean, M2), then
// the batch into the running stat with RunningStat.update, and writes the normalization
// constants (mean, std + 1e-8) -- a batched MeanStdFilter call pushes every row before
// normalizing.  (Round 2 ran one workgroup per column over all rows: 14.4 us per env-step at
// 4096 envs.  The same chunks merged by the last-arriving workgroup of a column -- agent-scope
// acq_rel atomics, one L2 write-back per workgroup -- measured 18.3 us.)
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_filter_chunk(const float* __restrict__ obs, int N, int D,
                                                      double* __restrict__ part) {
#include "filter_chunk_body.h"
}

__global__ void k_filter_merge(int N, int D, const double* __restrict__ part, double* n_run, double* M,
                               double* S, double* normc, int push, int enabled, double* dn, double* dM,
                               double* dS) {
#include "filter_merge_body.h"
}

size_t filter_part_doubles(int N, int D) { return (size_t)2 * D * ((N + FP_ROWS - 1) / FP_ROWS); }

void launch_filter_push(hipStream_t s, const float* obs, int N, int D, double* n_run, double* M,
                        double* S, double* normc, int update, int enabled, double* dn, double* dM,
                        double* dS, double* part) {
  const int push = enabled && update;
  if (push)
    hipLaunchKernelGGL(k_filter_chunk, dim3(D, (N + FP_ROWS - 1) / FP_ROWS), dim3(256), 0, s, obs, N, D, part);
  hipLaunchKernelGGL(k_filter_merge, dim3(1), dim3(64), 0, s, N, D, part, n_run, M, S, normc, push, enabled,
                     dn, dM, dS);
}

// a1: per-agent gather of the normalized observation into stage[p][c][f].
__global__ void k_observe_ffn(RouteArgs ra, const float* __restrict__ obs,
                              const double* __restrict__ normc, float clip, float* const* stage_tab,
                              const double* __restrict__ pf, FilterCount fc) {
  filter_count(fc);
#define OBSERVE_E0 ra.e0
#include "observe_ffn_body.h"
}

void launch_observe_ffn(hipStream_t s, const RouteArgs& ra, const float* obs, const double* normc,
                        float clip, float* const* stage, const double* pf, const FilterCount& fc) {
  int maxw = 0;
  for (int p = 0; p < ra.P; ++p) maxw = max(maxw, ra.N * ra.pol[p].k * ra.pol[p].d);
  dim3 grid((maxw + 255) / 256, ra.P);
  hipLaunchKernelGGL(k_observe_ffn, grid, dim3(256), 0, s, ra, obs, normc, clip, stage, pf, fc);
}

// ------------------------------------------------------------------------------------
// a2 (RLlib side): per-policy MeanStdFilter, unclipped (RLlib get_filter, clip=None).
// Policy p's rows at a step are its k agents' routed columns of every env, so the batch
// statistics of policy column f are sums of the env-normalized full-observation column
// statistics over the slots: one fp64 pass over obs [N][D] (k_zstats) serves every policy.
// The batch is merged with RunningStat.update (Chan), like the env-side filter.
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_zstats(const float* __restrict__ obs, int N, int D,
                                                const double* __restrict__ normc, float clip,
                                                double* __restrict__ zs) {
#include "zstats_body.h"
}

__global__ void k_pfilter(RouteArgs ra, const double* __restrict__ zs, double* pf, int update) {
#include "pfilter_body.h"
}

void launch_policy_filter(hipStream_t s, const RouteArgs& ra, const float* obs, const double* normc, float clip,
                          double* zs, double* pf, int update) {
  if (update) hipLaunchKernelGGL(k_zstats, dim3(ra.full_dim), dim3(256), 0, s, obs, ra.N, ra.full_dim, normc, clip, zs);
  hipLaunchKernelGGL(k_pfilter, dim3(ra.P), dim3(64), 0, s, ra, zs, pf, update);
}

// a3: graph observation X[env][node] = [normalized 19 features | ego quaternion (raw obs)].
__global__ void k_observe_gnn(RouteArgs ra, const float* __restrict__ obs,
                              const double* __restrict__ normc, float clip, float* __restrict__ X,
                              FilterCount fc) {
  filter_count(fc);
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= ra.N * 4) return;
  const int e = ra.e0 + (gid >> 2), n = gid & 3;
  const PolicyRoute& pr = ra.pol[0];
  const float* o = obs + (size_t)e * ra.full_dim;
  float* x = X + ((size_t)e * 4 + n) * 23;
  for (int f = 0; f < 19; ++f) {
    const int idx = pr.obs_index[n][f];
    x[f] = norm_obs(o[idx], normc, idx, clip);
  }
  // leg_encoding_ego: quat_mul(obs[1:5], [0, 0, sin(a/2), cos(a/2)]) in fp64
  const double rad = (double)ra.leg_angle[n] / 2.0 * (3.14159265358979323846 / 180.0);
  const double z2 = sin(rad), w2 = cos(rad);
  const double x1 = o[1], y1 = o[2], z1 = o[3], w1 = o[4];
  x[19] = (float)(x1 * w2 + y1 * z2 - z1 * 0.0 + w1 * 0.0);
  x[20] = (float)(-x1 * z2 + y1 * w2 + z1 * 0.0 + w1 * 0.0);
  x[21] = (float)(x1 * 0.0 - y1 * 0.0 + z1 * w2 + w1 * z2);
  x[22] = (float)(-x1 * 0.0 - y1 * 0.0 - z1 * z2 + w1 * w2);
}

void launch_observe_gnn(hipStream_t s, const RouteArgs& ra, const float* obs, const double* normc,
                        float clip, float* stage_x, const FilterCount& fc) {
  hipLaunchKernelGGL(k_observe_gnn, dim3((ra.N * 4 + 255) / 256), dim3(256), 0, s, ra, obs, normc,
                     clip, stage_x, fc);
}

// ------------------------------------------------------------------------------------
// a4 + a6 + a7: fused rollout forward.  Workgroup = 8 waves = 64 rows of ONE policy
// (grid.y = policy).  The policy's weights are staged once into LDS in the swizzled
// image; waves 0-3 run the policy branch and waves 4-7 the value branch of the same four
// 16-row tiles, from registers (MFMA 16x16x4 f32), so the two branch chains run side by side
// on each SIMD.  The policy waves sample a = mean + exp(log_std) * eps, compute logp, write
// the training record and scatter clip(a, -1, 1) into the env action vector.
// ------------------------------------------------------------------------------------
template <int A, int KS1>
__global__ void __launch_bounds__(512) k_act_ffn(RouteArgs ra, ActArgs aa) {
#define ACT(field) aa.field
#include "act_ffn_body.h"
}

template <int A, int KS1>
static void launch_act_t(hipStream_t s, dim3 grid, const RouteArgs& ra, const ActArgs& aa) {
  hipLaunchKernelGGL((k_act_ffn<A, KS1>), grid, dim3(512), LDS_WEIGHTS_FLOATS(2 * A) * 4, s, ra, aa);
}

void launch_act_ffn(hipStream_t s, const RouteArgs& ra, const ActArgs& aa) {
  const RowGeom g = row_geom(ra, aa.e1 - aa.e0);
  dim3 grid((g.rows + 63) / 64, ra.P);
  DDRL_DISPATCH_A_KS1(ra.A, g.d, launch_act_t, s, grid, ra, aa);
}

// ------------------------------------------------------------------------------------
// a8: per-leg (or global / normalized) reward of each agent; fp64 like the reference.
// ------------------------------------------------------------------------------------
// One thread per (env, agent): the agent's control cost and its bodies' contact cost.
__global__ void k_reward(RewardArgs ra, const float* __restrict__ fw, const float* __restrict__ cfrc,
                         const float* __restrict__ actions, const uint8_t* __restrict__ done,
                         uint8_t* __restrict__ done_tn) {
#define REWARD(field) ra.field
#define REWARD_DONE(e) (done ? done[e] : 0)   // done is optional: null records no episode ends
#include "reward_body.h"
}

void launch_reward(hipStream_t s, const RewardArgs& ra, const float* fw, const float* cfrc,
                   const float* actions, const uint8_t* done, uint8_t* done_tn) {
  const int n = ra.n * ra.n_agents;
  hipLaunchKernelGGL(k_reward, dim3((n + 255) / 256), dim3(256), 0, s, ra, fw, cfrc, actions,
                     done, done_tn);
}

int ffn_param_count(int d, int A) { return ffn_offsets(d, A).n; }

// ------------------------------------------------------------------------------------
// ModelV2.forward + value_function (fcnet_glorot_uniform_init.py:120-125) on n rows.
// ------------------------------------------------------------------------------------
template <int A, int KS1>
__global__ void __launch_bounds__(256) k_forward_ffn(ForwardArgs fa) {
  constexpr int O = 2 * A;
  extern __shared__ float lds[];
  NetLds PW, VW;
  stage_weights(fa.theta, fa.d, A, lds, PW, VW, 256);
  __syncthreads();
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 64 + 16 * w + c;
  const bool valid = row < fa.n;
  const int d = fa.d;
  float xop[12];
#pragma unroll
  for (int s = 0; s < 12; ++s) {
    const int f = 4 * s + q;
    xop[s] = (valid && s < KS1 && f < d) ? fa.x[(size_t)row * d + f] : 0.f;
  }
  floatx4 h1[4], h2[4];
  float vout[1], logits[O];
  ffn_branch_fwd<1, KS1>(VW, xop, h1, h2, vout);
  ffn_branch_fwd<O, KS1>(PW, xop, h1, h2, logits);
  if (!valid) return;
  if (fa.cup) {   // "cup": leg index of the row (clamped to the table; the host validates it)
    const int leg = min(max(fa.node[row], 0), 3);
#pragma unroll
    for (int j = 0; j < A; ++j) logits[j] *= fa.cup[leg * A + j];
  }
  if (q == 0) fa.values[row] = vout[0];
  for (int j = q; j < O; j += 4) fa.logits[(size_t)row * O + j] = logits[j];
}

template <int A, int KS1>
static void launch_forward_t(hipStream_t s, dim3 grid, const ForwardArgs& fa) {
  hipLaunchKernelGGL((k_forward_ffn<A, KS1>), grid, dim3(256), LDS_WEIGHTS_FLOATS(2 * A) * 4, s, fa);
}

void launch_forward_ffn(hipStream_t s, const ForwardArgs& fa) {
  dim3 grid((fa.n + 63) / 64);
  DDRL_DISPATCH_A_KS1(fa.A, fa.d, launch_forward_t, s, grid, fa);
}
