// Input sensitivity ("importance matrix") of a trained policy during evaluation: at every
// control step, every non-constant input feature f of every (env, slot) row is moved by
// -h_f / +h_f, the 2d perturbed rows go through the policy forward, and the differences of the
// clipped action means are accumulated in fp64.
//
// Reference: evaluation/rollout_episodes_compute_gradient.py:59-68 (the +-0.1 std perturbation of
// the filtered observation), :111-122 (2d compute_action(explore=False) calls per step,
// grads += act_high - act_low, grads_abs += |act_high - act_low|), :167-168 (the two .npy files).
//
// The rows of a 16x16x4 MFMA tile are independent of each other, so a perturbed row's logits
// are, bit for bit, the logits k_eval_act (eval.hip) produces for an observation carrying the
// same operand bits: the same ffn_fwd_rt instruction sequence per tile, the same LDS image.
#include "common.h"
#include "kernels.h"
#include "ffn.h"
#include "policy_io.h"

// after stage_policy_weights' LDS image (ffn.h): two buffers (iteration parity) of 48 base inputs
// + 96 perturbed inputs
#define SENS_XBUF 144
#define SENS_LDS_FLOATS(O) (((LDS_POLICY_FLOATS(O) + 3) & ~3) + 2 * SENS_XBUF)

// ------------------------------------------------------------------------------------
// Workgroup = 4 waves, the weights of ONE policy (grid.y) staged once; it then takes the base
// rows blockIdx.x, blockIdx.x + gridDim.x, ... of that policy.  A base row's 2d <= 96 perturbed
// rows are the rows of up to 6 tiles: perturbed row r = 2f + sign (sign 0: z_f - h_f, 1: z_f + h_f)
// is row r & 15 of tile r >> 4; wave w runs tiles w (and w + 4 when RT = 2, i.e. when 2d > 64).
//
// Per base row: threads 0..95 build the base input x_f and the perturbed input of their row in
// fp64 (the step is added to the env-normalized value, before the per-policy filter and before
// the rounding to fp32) and leave them in LDS; every lane then assembles its layer-1 operands
// X[row = c][f = 4s + q] from the base inputs, the one lane that holds the row's own feature
// taking the perturbed value.  The pair (minus, plus) of a feature sits in lanes c, c + 1: a
// DPP quad swap gives the difference.  Accumulators are per base row ([C][2][d][A] fp64, the
// row's lanes own their entries, launches are stream-ordered): no atomics, and the sum over rows
// is taken in row order by k_sens_reduce.
// ------------------------------------------------------------------------------------
template <int A, int KS1>
__global__ void __launch_bounds__(256) k_eval_sens(RouteArgs ra, EvalSensArgs sa) {
  constexpr int O = 2 * A;
  constexpr int RT = KS1 > 8 ? 2 : 1;   // d <= 32: 2d <= 64 rows fit the first four tiles
  extern __shared__ float lds[];
  const int p = blockIdx.y;
  const PolicyRoute& pr = ra.pol[p];
  const int row_hi = ra.N * pr.k;
  if ((int)blockIdx.x >= row_hi) return;
  const int d = pr.d, nrows = 2 * d;
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, q = lane >> 4, w = tid >> 6;
  const double* P = policy_filter_normc(sa.in.pf, p);
  const double* step = sa.step + (size_t)p * DDRL_MAXD;
  float* xbuf = lds + ((LDS_POLICY_FLOATS(O) + 3) & ~3);
  NetLds PW;
  stage_policy_weights(sa.in.theta[p], d, A, lds, PW, 256);
  // (the first __syncthreads of the loop also publishes the weights)
  int it = 0;   // base rows this workgroup has built inputs for (buffer parity)
  for (int b = blockIdx.x; b < row_hi; b += gridDim.x) {
    const int e = b / pr.k, slot = b - e * pr.k;
    const bool accum = sa.ep_count[e] < sa.E;   // the env is still below its episode quota
    if (!accum && !sa.means_out[p]) continue;   // workgroup-uniform
    float* xb = xbuf + (it & 1) * SENS_XBUF;    // [48] base inputs
    float* xp = xb + 48;                        // [96] the perturbed input of every row
    if (tid < 96) {
      const int f = tid >> 1;
      float vb = 0.f, vp = 0.f;
      if (f < d) {
        const int idx = pr.obs_index[slot][f];
        if (idx < 0) {
          vb = vp = const_input(idx);   // constants are not perturbed
        } else {
          const double z = norm_obs_d(sa.in.obs[(size_t)e * ra.full_dim + idx], sa.in.normc, idx, sa.in.clip);
          const double h = step[f];
          const double zp = (tid & 1) ? z + h : z - h;
          // policy_input (policy_io.h) of both values under one test of P: through the helper, and
          // through routed_input's two levels, the A = 2 instances measured up to 0.5 % slower
          if (P) {
            vb = (float)((z - P[2 * f]) / P[2 * f + 1]);
            vp = (float)((zp - P[2 * f]) / P[2 * f + 1]);
          } else {
            vb = (float)z;
            vp = (float)zp;
          }
        }
      }
      if (!(tid & 1)) xb[f] = vb;
      xp[tid] = vp;
    }
    // one barrier per base row: a wave that runs ahead writes the other buffer, and cannot reach
    // this one again before every wave has passed the next barrier, i.e. has read it
    __syncthreads();
    ++it;
    if (16 * w >= nrows) continue;   // wave-uniform: none of this wave's tiles holds a row
    float xop[RT][12];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int r = 16 * (w + 4 * t) + c;
      const bool valid = r < nrows;
      const int pf = valid ? r >> 1 : -1;       // the feature this row moves
      const float own = xp[valid ? r : 0];
#pragma unroll
      for (int s = 0; s < 12; ++s) {
        const int f = 4 * s + q;
        float v = 0.f;
        if (s < KS1 && f < d) v = f == pf ? own : xb[f];
        xop[t][s] = v;
      }
    }
    floatx4 h1[RT][4], h2[RT][4];
    float logits[RT][O];
    ffn_fwd_rt<O, KS1, RT>(PW, xop, h1, h2, logits);
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int r = 16 * (w + 4 * t) + c;
      const bool valid = r < nrows;
      const int f = valid ? r >> 1 : 0;
      const bool moved = valid && pr.obs_index[slot][f] >= 0;
      float mean[A], diff[A];
#pragma unroll
      for (int j = 0; j < A; ++j) {
        float mu = logits[t][j];
        // "cup" model: mean_j *= coupling[leg][j], leg = the base row's slot (k_eval_act)
        if (sa.in.cup[p]) mu *= sa.in.cup[p][slot * A + j];
        mean[j] = clip_action(mu);   // compute_action clips; explore=False: the mean
        // even lane c: minus row, lane c + 1: plus row
        diff[j] = dpp_mov<0xB1>(mean[j]) - mean[j];
      }
      if (moved && accum && !(c & 1)) {
        double* g = sa.acc[p] + (((size_t)b * 2) * d + f) * A;
        double* ga = g + (size_t)d * A;
#pragma unroll
        for (int j = 0; j < A; ++j)
          if ((j & 3) == q) {   // the four q lanes of a row hold the same means: they share the A entries
            const double dv = (double)diff[j];
            g[j] += dv;
            ga[j] += fabs(dv);
          }
      }
      if (valid && q == 1 && sa.means_out[p]) {
        float* mo = sa.means_out[p] + ((size_t)b * nrows + r) * A;
#pragma unroll
        for (int j = 0; j < A; ++j) mo[j] = moved ? mean[j] : __builtin_nanf("");
      }
    }
    if (accum && tid == 0) sa.rowcnt[p][b] += 1;
  }
}

template <int A, int KS1>
static void launch_eval_sens_t(hipStream_t s, dim3 grid, const RouteArgs& ra, const EvalSensArgs& sa) {
  hipLaunchKernelGGL((k_eval_sens<A, KS1>), grid, dim3(256), SENS_LDS_FLOATS(2 * A) * 4, s, ra, sa);
}

void launch_eval_sens(hipStream_t s, const RouteArgs& ra, const EvalSensArgs& sa, int grid_cap) {
  const RowGeom g = row_geom(ra, ra.N);
  dim3 grid(max(1, min(g.rows, grid_cap)), ra.P);
  DDRL_DISPATCH_A_KS1(ra.A, g.d, launch_eval_sens_t, s, grid, ra, sa);
}

// The sum over base rows, in row order: thread i owns entry i of [2][d][A]; thread 0 also adds
// the rows' step counts.
__global__ void __launch_bounds__(256) k_sens_reduce(const double* __restrict__ acc, const long long* __restrict__ rowcnt,
                                                    int C, int n, double* __restrict__ out, long long* __restrict__ rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    double s = 0.0;
    for (int r = 0; r < C; ++r) s += acc[(size_t)r * n + i];
    out[i] = s;
  }
  if (i == 0) {
    long long k = 0;
    for (int r = 0; r < C; ++r) k += rowcnt[r];
    rows[0] = k;
  }
}

void launch_sens_reduce(hipStream_t s, const double* acc, const long long* rowcnt, int C, int n, double* out,
                        long long* rows) {
  hipLaunchKernelGGL(k_sens_reduce, dim3((n + 255) / 256), dim3(256), 0, s, acc, rowcnt, C, n, out, rows);
}
