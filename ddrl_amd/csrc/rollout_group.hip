// Group rollout: the kernels of a device-plane training step (rollout.hip, devenv.hip) with a
// member axis.  M same-shaped contexts, each with its own device env plane, step side by side: the
// member is blockIdx.z, rows / envs / filter chunks are counted inside the member, and whatever
// differs between members (every pointer, the env's seed, time limit, target velocities and
// terrain) is read from a device table of RolloutMember, indexed by the wave-uniform blockIdx.z.
//
// Equality contract: member m's outputs are, bit for bit, what the plain kernels write for that
// context and env plane alone.  Each kernel below is the plain kernel's body over the same
// force-inlined pieces (stage_weights, ffn_branch_fwd, scatter_action, routed_input, norm_obs_d,
// agent_reward_d, envdyn.h's step pieces) in the same order, with the plain kernel's argument block
// replaced by the member's table entry.  The rollout kernels are compiled with the fp-contraction
// setting of rollout.hip (the HIP default); the env step with that of devenv.hip (off): envdyn.h
// is included below the pragma that turns it off, ahead of the step kernel.
#include "common.h"
#include "kernels.h"
#include "ffn.h"
#include "policy_io.h"

#define FP_ROWS 256   // rows per filter chunk, as rollout.hip

// ---- act: k_act_ffn with grid (ceil(n k_max / 64), P, M) ----
template <int A, int KS1>
__global__ void __launch_bounds__(512) k_act_ffn_group(RouteArgs ra, RolloutGroupArgs ga, int t, int bootstrap) {
  constexpr int O = 2 * A;
  extern __shared__ float lds[];
  const RolloutMember& mb = ga.tab[blockIdx.z];
  const int p = blockIdx.y;
  const PolicyRoute& pr = ra.pol[p];
  const int C = ga.C[p];
  const int row_hi = ga.n * pr.k;
  const int row0 = blockIdx.x * 64;
  if (row0 >= row_hi) return;
  const int d = pr.d;
  NetLds PW, VW;
  stage_weights(mb.theta[p], d, A, lds, PW, VW, 512);
  __syncthreads();

  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4, w = threadIdx.x >> 6;
  const bool value_wave = w >= 4;
  if (bootstrap && !value_wave) return;   // bootstrap: V(s_T) only
  const int row = row0 + 16 * (w & 3) + c;
  const bool valid = row < row_hi;
  const float* xs = mb.stage[p] + (size_t)(valid ? row : 0) * d;
  float xop[12];
#pragma unroll
  for (int s = 0; s < 12; ++s) {
    const int f = 4 * s + q;
    xop[s] = (s < KS1 && f < d && valid) ? xs[f] : 0.f;
  }
  floatx4 h1[4], h2[4];
  const RecLayout& L = ga.lay[p];
  if (value_wave) {
    float vout[1];
    ffn_branch_fwd<1, KS1>(VW, xop, h1, h2, vout);
    if (valid && q == 0) {
      if (bootstrap) mb.last_v[p][row] = vout[0];
      else mb.rec[p][((size_t)t * C + row) * L.stride + L.vf] = vout[0];
    }
    return;
  }
  float logits[O];
  ffn_branch_fwd<O, KS1>(PW, xop, h1, h2, logits);
  if (!valid) return;
  float* rp = mb.rec[p] + ((size_t)t * C + row) * L.stride;
  const int e = row / pr.k, slot = row - e * pr.k;
  const int agent = pr.agent[slot];
  const float* cup = mb.cup[p];
  if (cup) {
#pragma unroll
    for (int j = 0; j < A; ++j) logits[j] *= cup[slot * A + j];
  }
  // sample + logp (DiagGaussian, RLlib 1.0): a = mean + std * eps
  const float* eps_t = mb.eps + (size_t)t * ga.n * ra.n_agents * A;
  float logp = -0.5f * (float)(DDRL_LOG2PI * A);
  float act[A];
#pragma unroll
  for (int j = 0; j < A; ++j) {
    const float mu = logits[j], ls = logits[A + j];
    const float sd = expf(ls);
    const float eps = eps_t[((size_t)e * ra.n_agents + agent) * A + j];
    act[j] = mu + sd * eps;
    const float z = (act[j] - mu) / sd;
    logp -= 0.5f * z * z;
    logp -= ls;
  }
  // q-lanes split the record stores
  for (int f = q; f < d; f += 4) rp[L.obs + f] = xs[f];
  if (q == 0) {
#pragma unroll
    for (int j = 0; j < A; ++j) {
      rp[L.act + j] = act[j];
      scatter_action(mb.actions, pr, e, slot, j, act[j]);
    }
  } else if (q == 1) {
#pragma unroll
    for (int j = 0; j < O; ++j) rp[L.logit + j] = logits[j];
  } else if (q == 2) {
    rp[L.logp] = logp;
    if (L.cid >= 0) rp[L.cid] = (float)slot;
  }
}

template <int A, int KS1>
static void launch_act_group_t(hipStream_t s, dim3 grid, const RouteArgs& ra, const RolloutGroupArgs& ga, int t,
                               int bootstrap) {
  hipLaunchKernelGGL((k_act_ffn_group<A, KS1>), grid, dim3(512), LDS_WEIGHTS_FLOATS(2 * A) * 4, s, ra, ga, t, bootstrap);
}

static void launch_act_group(hipStream_t s, const RouteArgs& ra, const RolloutGroupArgs& ga, int t, int bootstrap) {
  const RowGeom g = row_geom(ra, ga.n);
  dim3 grid((g.rows + 63) / 64, ra.P, ga.M);
  DDRL_DISPATCH_A_KS1(ra.A, g.d, launch_act_group_t, s, grid, ra, ga, t, bootstrap);
}

// ---- reward: k_reward with grid (ceil(n n_agents / 256), 1, M) ----
__global__ void k_reward_group(RewardArgs ra, const RolloutMember* __restrict__ tab, int t) {
  const RolloutMember& mb = tab[blockIdx.z];
  const int na = ra.n_agents;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= ra.n * na) return;
  const int e = gid / na, j = gid - e * na;
  const double r = agent_reward_d(ra, j, (double)mb.env.fw[e], mb.env.cfrc + (size_t)e * 14 * 6, mb.actions + (size_t)e * 8);
  const int p = ra.policy_of_agent[j], slot = ra.slot_of_agent[j];
  const size_t C = (size_t)ra.N * ra.k[p];
  float* rp = mb.rec[p] + ((size_t)t * C + (size_t)e * ra.k[p] + slot) * ra.lay[p].stride;
  rp[ra.lay[p].rew] = (float)r;
  if (j == 0) mb.done_tn[(size_t)t * ra.N + e] = mb.env.done[e];
}

// ---- env-side filter push: k_filter_chunk / k_filter_merge, chunks counted from the member's first env ----
__global__ void __launch_bounds__(256) k_filter_chunk_group(const RolloutMember* __restrict__ tab, int N, int D) {
  const RolloutMember& mb = tab[blockIdx.z];
  const float* obs = mb.env.obs;
  const int j = blockIdx.x, sc = blockIdx.y;
  __shared__ double red[4];
  const int tid = threadIdx.x, w = tid >> 6;
  const int e = sc * FP_ROWS + tid;
  const int n_c = min(FP_ROWS, N - sc * FP_ROWS);
  const float x = e < N ? obs[(size_t)e * D + j] : 0.f;
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
    double* pc = mb.f_part + ((size_t)sc * D + j) * 2;
    pc[0] = mean_c;
    pc[1] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

__global__ void k_filter_merge_group(const RolloutMember* __restrict__ tab, int N, int D, int push, int enabled) {
  const RolloutMember& mb = tab[blockIdx.z];
  const int j = threadIdx.x;
  if (j >= D) return;
  const double* part = mb.f_part;
  double n1 = mb.f_n[0];
  double Mj = mb.f_M[j], Sj = mb.f_S[j];
  if (push) {
    // the batch's (mean, M2): the chunks merged in order (Chan et al.)
    const int nchunks = (N + FP_ROWS - 1) / FP_ROWS;
    double nb = 0.0, mean_b = 0.0, s_b = 0.0;
    for (int c = 0; c < nchunks; ++c) {
      const double* pc = part + ((size_t)c * D + j) * 2;
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
    mb.f_M[j] = Mj;
    mb.f_S[j] = Sj;
    // the same batch merged into the delta buffer (pushes since the last filter sync)
    double* dM = mb.f_dM;
    double* dS = mb.f_dS;
    const double d1 = mb.f_dn[0], dd = d1 + n2, ddl = dM[j] - mean_b;
    dM[j] = (d1 * dM[j] + n2 * mean_b) / dd;
    dS[j] = dS[j] + s_b + ddl * ddl * d1 * n2 / dd;
  }
  const double var = n1 > 1.0 ? Sj / (n1 - 1.0) : Mj * Mj;
  mb.f_normc[2 * j] = enabled ? Mj : 0.0;
  mb.f_normc[2 * j + 1] = enabled ? sqrt(var) + 1e-8 : 1.0;
}

// ---- per-policy filter: k_zstats / k_pfilter ----
__global__ void __launch_bounds__(256) k_zstats_group(const RolloutMember* __restrict__ tab, int N, int D, float clip) {
  const RolloutMember& mb = tab[blockIdx.z];
  const float* obs = mb.env.obs;
  const double* normc = mb.f_normc;
  const int j = blockIdx.x, tid = threadIdx.x;
  __shared__ double red[2][4];
  double s1 = 0.0, s2 = 0.0;
  for (int e = tid; e < N; e += 256) {
    const double z = norm_obs_d(obs[(size_t)e * D + j], normc, j, clip);
    s1 += z;
    s2 += z * z;
  }
  s1 = wave_sum_d(s1);
  s2 = wave_sum_d(s2);
  if ((tid & 63) == 0) { red[0][tid >> 6] = s1; red[1][tid >> 6] = s2; }
  __syncthreads();
  if (tid == 0) {
    mb.zs[2 * j] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    mb.zs[2 * j + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

__device__ __forceinline__ void chan_merge_g(double& n, double& M, double& S, double nb, double mb, double sb) {
  const double tot = n + nb, delta = M - mb;
  M = (n * M + nb * mb) / tot;
  S = S + sb + delta * delta * n * nb / tot;
}

__global__ void k_pfilter_group(RouteArgs ra, const RolloutMember* __restrict__ tab, int update) {
  const RolloutMember& mem = tab[blockIdx.z];
  const double* zs = mem.zs;
  const int p = blockIdx.x, f = threadIdx.x;
  const PolicyRoute& pr = ra.pol[p];
  double* P = mem.pf + (size_t)p * PF_STRIDE;
  const double n0 = P[PF_N], dn0 = P[PF_DN];
  const double nb = (double)ra.N * pr.k;
  __syncthreads();
  if (f < pr.d) {
    double M = P[PF_M + f], S = P[PF_S + f], n = n0;
    if (update) {
      double s1 = 0.0, s2 = 0.0;
      for (int s = 0; s < pr.k; ++s) {
        const int idx = pr.obs_index[s][f];
        s1 += zs[2 * idx];
        s2 += zs[2 * idx + 1];
      }
      const double mb = s1 / nb, sb = fmax(s2 - s1 * mb, 0.0);
      chan_merge_g(n, M, S, nb, mb, sb);
      double dn = dn0, dM = P[PF_DM + f], dS = P[PF_DS + f];
      chan_merge_g(dn, dM, dS, nb, mb, sb);
      P[PF_M + f] = M;
      P[PF_S + f] = S;
      P[PF_DM + f] = dM;
      P[PF_DS + f] = dS;
      n = n0 + nb;
    }
    const double var = n > 1.0 ? S / (n - 1.0) : M * M;
    P[PF_NORMC + 2 * f] = M;
    P[PF_NORMC + 2 * f + 1] = sqrt(var) + 1e-8;
  }
  __syncthreads();
  if (update && f == 0) {
    P[PF_N] = n0 + nb;
    P[PF_DN] = dn0 + nb;
  }
}

// ---- observe: k_observe_ffn with grid (ceil(n k d / 256), P, M) ----
// The count of the pushed batch is added here, by one thread of the member's first block: after
// the member's merge kernel (the only reader of the old count) and once per member.
__global__ void k_observe_ffn_group(RouteArgs ra, const RolloutMember* __restrict__ tab, float clip, int count) {
  const RolloutMember& mb = tab[blockIdx.z];
  if (count && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    mb.f_n[0] += (double)count;
    mb.f_dn[0] += (double)count;
  }
  const int p = blockIdx.y;
  const PolicyRoute& pr = ra.pol[p];
  const int C = ra.N * pr.k;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= C * pr.d) return;
  const int c = gid / pr.d, f = gid - c * pr.d;
  const int e = c / pr.k, slot = c - e * pr.k;
  mb.stage[p][(size_t)c * pr.d + f] =
      routed_input(pr, slot, f, mb.env.obs + (size_t)e * ra.full_dim, mb.f_normc, clip, policy_filter_normc(mb.pf, p));
}

// ---- env step: k_devenv_step (devenv.hip), four lanes per env, grid (ceil(4 n / 256), 1, M) ----
// The env index is counted inside the member, so the (seed, env, episode, generation) keying of
// resets, target-velocity draws and the height field is the member's own plane's.
#pragma clang fp contract(off)
#include "envdyn.h"

namespace {
using namespace envdyn;

template <int K>
__device__ __forceinline__ double quad_get(double v) { return dpp_mov_d<K * 0x55>(v); }

template <bool kTerrain, bool kTvEnv>
__global__ void __launch_bounds__(256) k_devenv_step_group(const RolloutMember* __restrict__ tab) {
  const RolloutMember& mb = tab[blockIdx.z];
  const DevEnvArgs& A = mb.env;
  const float* actions = mb.actions;
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int e = g >> 2, leg = g & 3;
  if (e >= A.N) return;
  const size_t N = A.N;
  double* const st = A.st + e;
  const int hip = 2 * leg, knee = hip + 1;
  Torso t{st[0 * N], st[1 * N], st[2 * N], st[3 * N], st[4 * N], st[5 * N], st[6 * N], st[7 * N], st[8 * N], st[9 * N]};
  double q_h = st[(10 + hip) * N], q_k = st[(10 + knee) * N];
  double qd_h = st[(18 + hip) * N], qd_k = st[(18 + knee) * N];
  double frc_h = 0.0, frc_k = 0.0;
  double tv = st[38 * N];
  int steps = A.steps[e];
  unsigned episode = A.episode[e];
  const double a_h = envdyn::clip_action(actions[(size_t)e * 8 + hip]), a_k = envdyn::clip_action(actions[(size_t)e * 8 + knee]);
  const double x0 = t.x;
  double force = 0.0, f0 = 0.0, f1 = 0.0, f2 = 0.0, f3 = 0.0;
  Ground ground{0, 0.0, 0.0};
  if constexpr (kTerrain)
    ground = ground_of(Terrain{A.ter_lo, A.ter_hi, A.ter_bump, A.ter_inv_bump, A.ter_gen}, A.seed, e, episode);
#pragma unroll 1
  for (int f = 0; f < kFrameSkip; ++f) {
    double push;
    if constexpr (kTerrain) leg_contact_on(ground, leg, t.x, t.y, t.z, t.vz, q_h, q_k, qd_h, force, push);
    else leg_contact(t.z, t.vz, q_h, q_k, qd_h, force, push);
    f0 = quad_get<0>(force); f1 = quad_get<1>(force); f2 = quad_get<2>(force); f3 = quad_get<3>(force);
    const double p0 = quad_get<0>(push), p1 = quad_get<1>(push), p2 = quad_get<2>(push), p3 = quad_get<3>(push);
    LegSums sums = leg_sums_zero();
    accum_leg(sums, 0, f0, p0);
    accum_leg(sums, 1, f1, p1);
    accum_leg(sums, 2, f2, p2);
    accum_leg(sums, 3, f3, p3);
    joint_step(hip, a_h, q_h, qd_h, frc_h);
    joint_step(knee, a_k, q_k, qd_k, frc_k);
    torso_step(t, sums);
  }
  ++steps;
  const bool d = unhealthy(t.z) || steps >= A.time_limit;

  // outputs of the step, before a done env is reset (the lane split of k_devenv_step)
  float* cf = A.cfrc + (size_t)e * 84;
  float* mine = cf + (2 + 3 * leg) * 6;
#pragma unroll
  for (int i = 0; i < 18; ++i) mine[i] = 0.f;
  foot_row(force, q_h, mine[12], mine[15], mine[17]);
  float share = 0.f;
  if (leg == 3) {
    share += torso_share(f0);
    share += torso_share(f1);
    share += torso_share(f2);
    share += torso_share(f3);
  }
  cf[3 * leg] = 0.f;
  cf[3 * leg + 1] = 0.f;
  cf[3 * leg + 2] = share;
  float* kn = A.kin + (size_t)e * 9;
  kn[1 + hip] = (float)qd_h;
  kn[1 + knee] = (float)qd_k;
  if (leg == 0) {
    kn[0] = (float)(t.x - x0);
    A.fw[e] = forward_reward(t.x, x0, tv, A.D);
    A.done[e] = d ? 1 : 0;
  }

  // a done env starts its next episode at once
  double c_h = a_h, c_k = a_k;
  if (d) {
    episode += 1;
    steps = 0;
    if constexpr (kTvEnv) tv = A.tv_env[e];
    else tv = draw_tv(A.seed, e, episode, A.tv_list, A.n_tv);
    t = Torso{0.0, 0.0, reset_z(A.seed, e, episode), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    q_h = reset_q(A.seed, e, episode, hip); q_k = reset_q(A.seed, e, episode, knee);
    qd_h = reset_qd(A.seed, e, episode, hip); qd_k = reset_qd(A.seed, e, episode, knee);
    frc_h = 0.0; frc_k = 0.0; force = 0.0;
    c_h = 0.0; c_k = 0.0;
  }

  // the observation: one of the quaternion's four sin / cos per lane, exchanged like the forces
  const double half = 0.5 * (leg < 2 ? t.roll : t.pitch);
  const double trig = (leg & 1) ? sin(half) : cos(half);
  double w[4];
  quat_of(quad_get<0>(trig), quad_get<1>(trig), quad_get<2>(trig), quad_get<3>(trig), w);
  float* o = A.obs + (size_t)e * A.D;
  o[kObsQ + hip] = (float)q_h; o[kObsQ + knee] = (float)q_k;
  o[kObsQd + hip] = (float)qd_h; o[kObsQd + knee] = (float)qd_k;
  o[kObsFrc + hip] = (float)frc_h; o[kObsFrc + knee] = (float)frc_k;
  o[kObsCtrl + hip] = (float)c_h; o[kObsCtrl + knee] = (float)c_k;
  if (leg == 0) {
    o[0] = (float)t.z; o[1] = (float)w[0]; o[2] = (float)w[1];
  } else if (leg == 1) {
    o[3] = (float)w[2]; o[4] = (float)w[3]; o[kObsVel] = (float)t.vx;
  } else if (leg == 2) {
    o[kObsVel + 1] = (float)t.vy; o[kObsVel + 2] = (float)t.vz; o[kObsVel + 3] = (float)t.wroll;
  } else {
    o[kObsVel + 4] = (float)t.wpitch; o[kObsVel + 5] = (float)0.0;
    if (A.D > 43) o[kObsTv] = (float)tv;
  }

  // the state: own joints and foot; the torso's ten fields, tv and the counters split over the quad
  st[(10 + hip) * N] = q_h; st[(10 + knee) * N] = q_k;
  st[(18 + hip) * N] = qd_h; st[(18 + knee) * N] = qd_k;
  st[(26 + hip) * N] = frc_h; st[(26 + knee) * N] = frc_k;
  st[(34 + leg) * N] = force;
  const double tf[10] = {t.x, t.y, t.z, t.vx, t.vy, t.vz, t.roll, t.pitch, t.wroll, t.wpitch};
  if (leg == 0) {
    st[0 * N] = tf[0]; st[4 * N] = tf[4]; st[8 * N] = tf[8];
  } else if (leg == 1) {
    st[1 * N] = tf[1]; st[5 * N] = tf[5]; st[9 * N] = tf[9];
  } else if (leg == 2) {
    st[2 * N] = tf[2]; st[6 * N] = tf[6]; st[38 * N] = tv;
  } else {
    st[3 * N] = tf[3]; st[7 * N] = tf[7];
    A.steps[e] = steps;
    A.episode[e] = episode;
  }
}

void launch_devenv_step_group(hipStream_t s, const RolloutGroupArgs& ga) {
  const dim3 grid((4 * ga.n + 255) / 256, 1, ga.M);
  if (ga.tv_env) {
    if (ga.ter_on) hipLaunchKernelGGL((k_devenv_step_group<true, true>), grid, dim3(256), 0, s, ga.tab);
    else hipLaunchKernelGGL((k_devenv_step_group<false, true>), grid, dim3(256), 0, s, ga.tab);
  } else {
    if (ga.ter_on) hipLaunchKernelGGL((k_devenv_step_group<true, false>), grid, dim3(256), 0, s, ga.tab);
    else hipLaunchKernelGGL((k_devenv_step_group<false, false>), grid, dim3(256), 0, s, ga.tab);
  }
}

}  // namespace

void launch_rollout_group_step(hipStream_t s, const RouteArgs& ra, const RewardArgs& rw, const RolloutGroupArgs& ga, int t) {
  const int n = ga.n, D = ra.full_dim, M = ga.M;
  launch_act_group(s, ra, ga, t, 0);
  launch_devenv_step_group(s, ga);
  hipLaunchKernelGGL(k_reward_group, dim3((n * rw.n_agents + 255) / 256, 1, M), dim3(256), 0, s, rw, ga.tab, t);
  const int push = ga.filter_enabled && ga.filter_update;
  if (push)
    hipLaunchKernelGGL(k_filter_chunk_group, dim3(D, (n + FP_ROWS - 1) / FP_ROWS, M), dim3(256), 0, s, ga.tab, n, D);
  hipLaunchKernelGGL(k_filter_merge_group, dim3(1, 1, M), dim3(64), 0, s, ga.tab, n, D, push, ga.filter_enabled);
  if (ga.policy_filter) {
    hipLaunchKernelGGL(k_zstats_group, dim3(D, 1, M), dim3(256), 0, s, ga.tab, n, D, ga.clip);
    hipLaunchKernelGGL(k_pfilter_group, dim3(ra.P, 1, M), dim3(64), 0, s, ra, ga.tab, 1);
  }
  int maxw = 0;
  for (int p = 0; p < ra.P; ++p) maxw = max(maxw, n * ra.pol[p].k * ra.pol[p].d);
  hipLaunchKernelGGL(k_observe_ffn_group, dim3((maxw + 255) / 256, ra.P, M), dim3(256), 0, s, ra, ga.tab, ga.clip,
                     push ? n : 0);
}

void launch_rollout_group_bootstrap(hipStream_t s, const RouteArgs& ra, const RolloutGroupArgs& ga) {
  launch_act_group(s, ra, ga, 0, 1);
}
