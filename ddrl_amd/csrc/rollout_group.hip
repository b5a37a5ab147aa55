// Group rollout: the kernels of a device-plane training step (rollout.hip, devenv.hip) with a
// member axis.  M same-shaped contexts, each with its own device env plane, step side by side: the
// member is blockIdx.z, rows / envs / filter chunks are counted inside the member, and whatever
// differs between members (every pointer, the env's seed, time limit, target velocities and
// terrain) is read from a device table of RolloutMember, indexed by the wave-uniform blockIdx.z.
//
// Equality contract: member m's outputs are, bit for bit, what the plain kernels write for that
// context and env plane alone.  It holds by construction: every kernel body is one text (*_body.h)
// that the plain unit and this one include inside the kernel's braces.  A kernel here is a signature
// and a prologue that names the text's operands from the member's table entry and the by-value group
// arguments (locals or references of the plain kernel's parameter names; accessor macros for the
// by-value blocks of act, reward and observe), and nothing after it.  A reference (const auto&) leaves
// the scalar load of the entry's field where the text reads the operand, a local puts it at the top
// of the kernel: each prologue uses what keeps the assembly the measured numbers were taken on
// (DESIGN.md "Population rollout").  The rollout texts are compiled with rollout.hip's fp-contraction
// setting (the HIP default); envdyn.h and the step text, included below the pragma, with devenv.hip's (off).
#include "common.h"
#include "kernels.h"
#include "ffn.h"
#include "policy_io.h"

// ---- act: k_act_ffn with grid (ceil(n k_max / 64), P, M) ----
template <int A, int KS1>
__global__ void __launch_bounds__(512) k_act_ffn_group(RouteArgs ra, RolloutGroupArgs ga, int t, int bootstrap) {
  const RolloutMember& mb = ga.tab[blockIdx.z];
  // act_<field>: where the group keeps that field of ActArgs
  const auto &act_theta = mb.theta, &act_cup = mb.cup;
  const auto &act_stage = mb.stage, &act_rec = mb.rec, &act_last_v = mb.last_v;
  const auto& act_lay = ga.lay;
  const auto& act_C = ga.C;
  const auto& act_actions = mb.actions;
  const int act_e0 = 0, act_e1 = ga.n, act_t = t, act_bootstrap = bootstrap;
  // the step's noise: a macro, formed where the text reads it (a local moves its loads ahead of the staging)
#define act_eps (mb.eps + (size_t)t * ga.n * ra.n_agents * A)
#define ACT(field) act_##field
#include "act_ffn_body.h"
#undef act_eps
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
  const auto &fw = mb.env.fw, &cfrc = mb.env.cfrc, &actions = mb.actions;
  const auto& done_tn = mb.done_tn;
  const auto& reward_rec = mb.rec;
  const int reward_e0 = 0, reward_t = t;
#define REWARD(field) reward_##field
#define REWARD_DONE(e) mb.env.done[e]   // a device env plane always has its done flags
#include "reward_body.h"
}

// ---- env-side filter push: k_filter_chunk / k_filter_merge, chunks counted from the member's first env ----
__global__ void __launch_bounds__(256) k_filter_chunk_group(const RolloutMember* __restrict__ tab, int N, int D) {
  const RolloutMember& mb = tab[blockIdx.z];
  const auto& obs = mb.env.obs;
  const auto& part = mb.f_part;
#include "filter_chunk_body.h"
}

__global__ void k_filter_merge_group(const RolloutMember* __restrict__ tab, int N, int D, int push, int enabled) {
  const RolloutMember& mb = tab[blockIdx.z];
  const double* part = mb.f_part;
  const auto &n_run = mb.f_n, &M = mb.f_M, &S = mb.f_S, &normc = mb.f_normc;
  const auto &dn = mb.f_dn, &dM = mb.f_dM, &dS = mb.f_dS;
#include "filter_merge_body.h"
}

// ---- per-policy filter: k_zstats / k_pfilter ----
__global__ void __launch_bounds__(256) k_zstats_group(const RolloutMember* __restrict__ tab, int N, int D, float clip) {
  const RolloutMember& mb = tab[blockIdx.z];
  const float* obs = mb.env.obs;
  const double* normc = mb.f_normc;
  const auto& zs = mb.zs;
#include "zstats_body.h"
}

__global__ void k_pfilter_group(RouteArgs ra, const RolloutMember* __restrict__ tab, int update) {
  const RolloutMember& mem = tab[blockIdx.z];   // the text has a local mb
  const double* zs = mem.zs;
  double* pf = mem.pf;
#include "pfilter_body.h"
}

// ---- observe: k_observe_ffn with grid (ceil(n k d / 256), P, M) ----
// The count of the pushed batch is added here, by one thread of the member's first block: after
// the member's merge kernel (the only reader of the old count) and once per member.
__global__ void k_observe_ffn_group(RouteArgs ra, const RolloutMember* __restrict__ tab, float clip, int count) {
  const RolloutMember& mb = tab[blockIdx.z];
  filter_count(FilterCount{mb.f_n, mb.f_dn, count});
  const auto& obs = mb.env.obs;
  const auto &normc = mb.f_normc, &pf = mb.pf;
  const auto& stage_tab = mb.stage;
#define OBSERVE_E0 0
#include "observe_ffn_body.h"
}

// ---- env step: k_devenv_step (devenv.hip), four lanes per env, grid (ceil(4 n / 256), 1, M) ----
// The env index is counted inside the member, so the (seed, env, episode, generation) keying of
// resets, target-velocity draws and the height field is the member's own plane's.
#pragma clang fp contract(off)
#include "envdyn.h"
#include "devenv_step.h"

namespace {
using namespace envdyn;

template <bool kTerrain, bool kTvEnv>
__global__ void __launch_bounds__(256) k_devenv_step_group(const RolloutMember* __restrict__ tab) {
  const RolloutMember& mb = tab[blockIdx.z];
  const DevEnvArgs& A = mb.env;
  const float* actions = mb.actions;
#include "devenv_step_body.h"
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
