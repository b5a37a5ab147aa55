// Evaluation members: M parameter sets evaluated side by side on one context, n envs each (the
// reference's sweeps -- evaluation/evaluate_trained_policies_pd.py:84-127 and
// evaluate_trained_policies_tvel_range_pd.py:52-78 roll out one restored agent per cell).  Member
// m owns the envs [m n, (m + 1) n); its weights, env-side filter and per-policy filter constants
// live at base + m * stride (kernels.h EvalMembersArgs).  The kernels here are k_eval_act
// (eval.hip) and the env-side filter push (rollout.hip) with the member in the grid, built from
// the same inlined pieces in the same order, so a member computes what a plain context of n envs
// holding its state computes, bit for bit.
#include "common.h"
#include "kernels.h"
#include "ffn.h"
#include "policy_io.h"

// ------------------------------------------------------------------------------------
// Fused evaluation forward of every member.  Workgroup = 4 waves = up to 64 rows of ONE policy
// (grid.y) of ONE member (grid.z), that member's policy branch staged into LDS; rows are counted
// within the member, the env of a row is m n + row / k.  A wave whose 16-row tile lies past the
// member's last row helps to stage the weights, meets the barrier and leaves before the MFMAs.
// ------------------------------------------------------------------------------------
template <int A, int KS1>
__global__ void __launch_bounds__(256) k_eval_act_members(RouteArgs ra, EvalMembersArgs ma) {
  constexpr int O = 2 * A;
  extern __shared__ float lds[];
  const int p = blockIdx.y, m = blockIdx.z;
  const PolicyRoute& pr = ra.pol[p];
  const int row_hi = ra.N * pr.k;
  const int row0 = blockIdx.x * 64;
  if (row0 >= row_hi) return;
  const int d = pr.d;
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4, w = threadIdx.x >> 6;
  const int row = row0 + 16 * w + c;
  const bool valid = row < row_hi;
  const int rv = valid ? row : 0;
  const int el = rv / pr.k, slot = rv - el * pr.k;
  const int e = m * ra.N + el;
  const float* o = ma.obs + (size_t)e * ra.full_dim;
  const double* normc = ma.filt + (size_t)m * FM_STRIDE + FM_NORMC;
  const double* P = policy_filter_normc(ma.pf ? ma.pf + (size_t)m * ma.pf_stride : nullptr, p);
  float xop[12];
#pragma unroll
  for (int s = 0; s < 12; ++s) {
    const int f = 4 * s + q;
    float v = 0.f;
    if (s < KS1 && f < d && valid) v = routed_input(pr, slot, f, o, normc, ma.clip, P);
    xop[s] = v;
  }
  const float* th = ma.theta[p] + (size_t)m * ma.theta_stride[p];
  NetLds PW;
  stage_policy_weights(th, d, A, lds, PW, 256);
  __syncthreads();
  if (row0 + 16 * w >= row_hi) return;   // wave-uniform: an empty tile, and no barrier follows
  floatx4 h1[4], h2[4];
  float logits[O];
  ffn_branch_fwd<O, KS1>(PW, xop, h1, h2, logits);
  if (!valid) return;
  const int agent = pr.agent[slot];
  // "cup" model: mean_j *= coupling[leg][j] (in place, as in k_eval_act)
  if (ma.cup_off[p] >= 0) {
    const float* cup = th + ma.cup_off[p];
#pragma unroll
    for (int j = 0; j < A; ++j) logits[j] *= cup[slot * A + j];
  }
  if (q == 0) {
#pragma unroll
    for (int j = 0; j < A; ++j) {
      const float mu = logits[j], ls = logits[A + j];
      float act = mu;   // deterministic: the DiagGaussian mean (explore=False)
      if (ma.eps) {
        const float sd = expf(ls);
        const float eps = ma.eps[((size_t)e * ra.n_agents + agent) * A + j];
        act = mu + sd * eps;
      }
      scatter_action(ma.actions, pr, e, slot, j, act);
    }
  } else if (q == 1 && ma.logits_out[p]) {
    float* lo = ma.logits_out[p] + ((size_t)m * row_hi + row) * O;
#pragma unroll
    for (int j = 0; j < O; ++j) lo[j] = logits[j];
  }
}

template <int A, int KS1>
static void launch_eval_act_members_t(hipStream_t s, dim3 grid, const RouteArgs& ra, const EvalMembersArgs& ma) {
  hipLaunchKernelGGL((k_eval_act_members<A, KS1>), grid, dim3(256), LDS_POLICY_FLOATS(2 * A) * 4, s, ra, ma);
}

void launch_eval_act_members(hipStream_t s, const RouteArgs& ra, const EvalMembersArgs& ma, int n_members) {
  const RowGeom g = row_geom(ra, ra.N);
  dim3 grid((g.rows + 63) / 64, ra.P, n_members);
  DDRL_DISPATCH_A_KS1(ra.A, g.d, launch_eval_act_members_t, s, grid, ra, ma);
}

// ------------------------------------------------------------------------------------
// Env-side MeanStdFilter push of every member: k_filter_chunk / k_filter_merge (rollout.hip) with
// the member in the grid.  Chunks of FP_ROWS rows are counted from the member's first env and
// merged in order with the same expressions.  The merge kernel also advances the member's counts
// (the plain path leaves that to the kernel behind it): its 64 lanes read the counts, meet a
// barrier, and lane 0 writes them.
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_filter_chunk_members(const float* __restrict__ obs, int N, int D,
                                                              double* __restrict__ part, size_t part_stride) {
  const int j = blockIdx.x, sc = blockIdx.y, m = blockIdx.z;
  __shared__ double red[4];
  const int tid = threadIdx.x, w = tid >> 6;
  const int e = sc * FP_ROWS + tid;   // within the member
  const int n_c = min(FP_ROWS, N - sc * FP_ROWS);
  const float x = e < N ? obs[((size_t)m * N + e) * D + j] : 0.f;
  double acc = wave_sum_d((double)x);
  if ((tid & 63) == 0) red[w] = acc;
  __syncthreads();
  const double mean_c = ((red[0] + red[1]) + (red[2] + red[3])) / (double)n_c;
  __syncthreads();
  const double dlt = e < N ? (double)x - mean_c : 0.0;
  acc = wave_sum_d(dlt * dlt);
  if ((tid & 63) == 0) red[w] = acc;
  __syncthreads();
  if (tid == 0) {
    double* pc = part + (size_t)m * part_stride + ((size_t)sc * D + j) * 2;
    pc[0] = mean_c;
    pc[1] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

__global__ void __launch_bounds__(64) k_filter_merge_members(int N, int D, const double* __restrict__ part,
                                                             size_t part_stride, double* filt, int push, int enabled) {
  const int j = threadIdx.x, m = blockIdx.x;
  double* F = filt + (size_t)m * FM_STRIDE;
  const double* pm = part + (size_t)m * part_stride;
  const double n0 = F[FM_N], d0 = F[FM_DN];
  if (j < D) {
    double n1 = n0;
    double Mj = F[FM_M + j], Sj = F[FM_S + j];
    if (push) {
      // the batch's (mean, M2): the chunks merged in order (Chan et al.)
      const int nchunks = (N + FP_ROWS - 1) / FP_ROWS;
      double nb = 0.0, mean_b = 0.0, s_b = 0.0;
      for (int c = 0; c < nchunks; ++c) {
        const double* pc = pm + ((size_t)c * D + j) * 2;
        const double nc = (double)min(FP_ROWS, N - c * FP_ROWS), nn = nb + nc, d = pc[0] - mean_b;
        mean_b = (nb * mean_b + nc * pc[0]) / nn;
        s_b = s_b + pc[1] + d * d * nb * nc / nn;
        nb = nn;
      }
      const double n2 = (double)N, n = n1 + n2;
      const double delta = Mj - mean_b;
      Mj = (n1 * Mj + n2 * mean_b) / n;
      Sj = Sj + s_b + delta * delta * n1 * n2 / n;
      n1 = n;
      F[FM_M + j] = Mj;
      F[FM_S + j] = Sj;
      // the same batch merged into the delta stat
      const double d1 = d0, dd = d1 + n2, ddl = F[FM_DM + j] - mean_b;
      F[FM_DM + j] = (d1 * F[FM_DM + j] + n2 * mean_b) / dd;
      F[FM_DS + j] = F[FM_DS + j] + s_b + ddl * ddl * d1 * n2 / dd;
    }
    const double var = n1 > 1.0 ? Sj / (n1 - 1.0) : Mj * Mj;
    F[FM_NORMC + 2 * j] = enabled ? Mj : 0.0;
    F[FM_NORMC + 2 * j + 1] = enabled ? sqrt(var) + 1e-8 : 1.0;
  }
  __syncthreads();   // every column has read the counts
  if (push && j == 0) {
    F[FM_N] = n0 + (double)N;
    F[FM_DN] = d0 + (double)N;
  }
}

void launch_filter_push_members(hipStream_t s, const float* obs, int n, int D, int n_members, double* filt,
                                int update, int enabled, double* part) {
  const int push = enabled && update;
  const size_t part_stride = filter_part_doubles(n, D);
  if (push)
    hipLaunchKernelGGL(k_filter_chunk_members, dim3(D, (n + FP_ROWS - 1) / FP_ROWS, n_members), dim3(256), 0, s, obs,
                       n, D, part, part_stride);
  hipLaunchKernelGGL(k_filter_merge_members, dim3(n_members), dim3(64), 0, s, n, D, part, part_stride, filt, push,
                     enabled);
}
