// What the capi_*.cpp files share (internal: not installed): the error helpers, the context and what it owns, the
// device allocation helpers and the helpers that cross files, all in namespace ddrl_impl.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/ddrl_hip.h"
#include "hostenv.h"
#include "kernels.h"

namespace ddrl_impl {
int fail(const std::string& msg);   // sets the thread's ddrl_last_error (capi_ctx.cpp), returns -1

// Zeroed device memory, 16 bytes at least: what every owner's allocation goes through.  On failure nothing stays
// allocated and *p is not written; `step`, where asked for, names the call that failed.
inline hipError_t dev_zalloc(void** p, size_t bytes, const char** step = nullptr) {
  bytes = std::max<size_t>(bytes, 16);
  void* ptr = nullptr;
  const char* at = "hipMalloc";
  hipError_t e = hipMalloc(&ptr, bytes);
  if (e == hipSuccess && (e = hipMemset(ptr, 0, bytes)) != hipSuccess) {
    at = "hipMemset";
    (void)hipFree(ptr);
  }
  if (step) *step = at;
  if (e == hipSuccess) *p = ptr;
  return e;
}
}  // namespace ddrl_impl

#define HIPCHK(x)                                                                   \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess)                                                           \
      return fail(std::string(#x) + ": " + hipGetErrorString(e_));                  \
  } while (0)

#define NCCLCHK(x)                                                                  \
  do {                                                                              \
    ncclResult_t r_ = (x);                                                          \
    if (r_ != ncclSuccess) return fail(std::string(#x) + ": " + ncclGetErrorString(r_)); \
  } while (0)

#define CHK_CTX(c) \
  if (!(c)) return fail("null context")

#define CHK_PID(c, pid) \
  if ((pid) < 0 || (pid) >= (c)->cfg.n_policies) return fail("bad policy id")

namespace ddrl_impl {
struct Policy {
  int k = 0, d = 0, C = 0, n_params = 0, R = 0, nb = 0;
  int agents[DDRL_MAXAG] = {0};
  RecLayout lay{};
  float *theta = nullptr, *m = nullptr, *v = nullptr, *beta_pow = nullptr;
  float *rec = nullptr, *stage = nullptr, *last_v = nullptr, *adv_norm = nullptr;
  float *stats = nullptr, *grad = nullptr;
  double* partials = nullptr;
  int last_steps = 0;
  size_t stats_steps = 0;   // rows of `stats` (num_sgd_iter * nb; peer mode may grow it)
};

// A group's device table of per-member kernel arguments, rebuilt at every run in a pinned host array and copied on
// the group's stream.  That array is the source of the copy: host() waits for `copied`, recorded behind the copy.
template <class T>
struct MemberTable {
  T *pinned = nullptr, *dev = nullptr;
  hipEvent_t copied = nullptr;
  int copy_pending = 0;
  bool alloc(size_t n) {
    const size_t bytes = n * sizeof(T);
    return hipHostMalloc((void**)&pinned, bytes, hipHostMallocDefault) == hipSuccess && dev_zalloc((void**)&dev, bytes) == hipSuccess &&
           hipEventCreateWithFlags(&copied, hipEventDisableTiming) == hipSuccess;
  }
  int host(T*& out) {
    if (copy_pending) HIPCHK(hipEventSynchronize(copied));
    copy_pending = 0;
    out = pinned;
    return 0;
  }
  int upload(hipStream_t stream, size_t n) {
    HIPCHK(hipMemcpyAsync(dev, pinned, n * sizeof(T), hipMemcpyHostToDevice, stream));
    HIPCHK(hipEventRecord(copied, stream));
    copy_pending = 1;
    return 0;
  }
  void stream_synced() { copy_pending = 0; }   // the caller has synchronized the stream of the last upload
  void release() {
    if (copied) (void)hipEventDestroy(copied);
    if (pinned) (void)hipHostFree(pinned);
    if (dev) (void)hipFree(dev);
  }
};

// A group's pinned staging buffer of device-to-host copies: many copies are enqueued into it, waited for once and
// handed to the caller's (pageable) arrays by the host.  fit() keeps the old contents of nothing: call it before the
// copies, with nothing in flight into the buffer.
struct PinnedStage {
  char* p = nullptr;
  size_t cap = 0;
  int fit(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    const size_t want = std::max(bytes, 2 * cap);
    cap = 0;
    HIPCHK(hipHostMalloc((void**)&p, want, hipHostMallocDefault));
    cap = want;
    return 0;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

// the member tables of the group fills a context led (device randomness, capi_rng.cpp)
struct RngTables {
  MemberTable<NoiseMember> noise;
  MemberTable<ScheduleMember> sched;
  int noise_cap = 0, sched_cap = 0;
};

inline void rng_tables_free(RngTables* t) {
  if (t->noise_cap) t->noise.release();
  if (t->sched_cap) t->sched.release();
  delete t;
}
}  // namespace ddrl_impl

using namespace ddrl_impl;   // (every file that includes this is one of the library's own)

struct ddrl_ctx {
  ddrl_cfg cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  Policy pol[DDRL_MAXP];
  RouteArgs route{};
  double *f_n = nullptr, *f_M = nullptr, *f_S = nullptr, *f_normc = nullptr;
  double *f_dn = nullptr, *f_dM = nullptr, *f_dS = nullptr;   // pushes since the last sync
  double* f_part = nullptr;                                     // filter push chunk scratch
  double* pf = nullptr;   // per-policy RLlib MeanStdFilter state [P][PF_STRIDE]
  double* zs = nullptr;   // fp64 column sums of the env-normalized observation [2][D]
  uint8_t* done_tn = nullptr;
  float** stage_tab = nullptr;    // device array of per-policy stage pointers
  int32_t* zero_perm = nullptr;
  unsigned long long* xchg = nullptr;  // norm^2 exchange granules of the update kernel
  unsigned long long* gx = nullptr;    // partial-gradient granules of the row-split update
  unsigned upd_epoch = 0;              // update launches so far (granule tag epochs)
  int update_split = 2;                // workgroups per branch of the fused update (1 or 2)
  int* err = nullptr;                  // device error word (exchange timeout)
  // Placement / rollback (fcnet update): the XCC of every block of the last update launch,
  // the exchange protocol (0: plain stores into the XCD's L2, 1: relaxed agent-scope atomics,
  // chosen by DDRL_XCHG=atomic or after a placement failure), and per policy a snapshot of
  // theta | m | v | beta powers taken before each update, restored when the launch fails.
  int* xcc = nullptr;
  int xchg_atomic = 0;
  int xcc_pending = 0;                 // blocks of an update launch not yet checked (grid size)
  int xcc_ksp = 2;
  int xcc_mask = 0;
  int fail_step = -1;                  // test hook: DDRL_TEST_FAIL_STEP
  float* snap[DDRL_MAXP] = {nullptr};
  int snap_mask = 0;
  float kl_last[DDRL_MAXP] = {0};
  GnnScratch gnn{};               // GraphNet step scratch (per-tile partial gradients, ...)
  // host-variant staging
  float *h_obs = nullptr, *h_eps = nullptr, *h_act = nullptr;
  ncclComm_t comm = nullptr;           // data-parallel learner (ddrl_comm_init)
  float* ddp_chunk = nullptr;          // ddrl_ppo_update_ddp: pre-gathered records of a run of steps
  size_t ddp_chunk_n = 0;
  int32_t* ddp_slots = nullptr;        // ... and the minibatch slot of every step (device copy)
  size_t ddp_slots_n = 0;
  std::vector<int32_t> ddp_slots_host; // source of that copy, alive until the call's final sync
  float *h_fw = nullptr, *h_cfrc = nullptr;
  uint8_t* h_done = nullptr;
  // ddrl_rollout_fragment as one HIP graph (T x (act, reward, filter push, observe) +
  // bootstrap), captured on first use and re-used while the call's buffers are the same
  // (every other kernel argument is fixed at context creation); DDRL_ROLLOUT_GRAPH=0: launches
  int rollout_graph = 1;
  hipGraphExec_t rg_exec = nullptr;
  hipStream_t cap_stream = nullptr;    // capture only (the caller's stream may be the null stream)
  const void* rg_key[6] = {nullptr};
  // peer mode (ddrl_ppo_update_peer): the outboxes shared with the peer context, this context's
  // row half, the launch tags both contexts step in lockstep, the IPC mapping to close, and the
  // per-rank virtual shuffle ([nb][128] row indices, this rank's rows in half peer_rank)
  void* peer_gx = nullptr;
  int peer_rank = -1;
  unsigned peer_epoch = 0;
  unsigned peer_steps = 0;   // steps the attached pair has run (the quads' tag bit and outbox parity)
  int peer_inflight = 0;     // a peer launch is enqueued and not yet checked (check_err)
  void* peer_ipc = nullptr;
  int32_t* peer_vsh = nullptr;
  size_t peer_vsh_n = 0;
  // evaluation (ddrl_eval_*): per-env fp64 accumulators, episode counts, the result table
  // [N][E][6], the two progress counters and the device copy of the env plane's kin buffer;
  // ev_normc_ok: the filter constants are known current (no push since they were written)
  int ev_on = 0;
  ddrl_eval_cfg ev_cfg{};
  double *ev_acc = nullptr, *ev_table = nullptr;
  int32_t* ev_count = nullptr;
  unsigned long long* ev_ctr = nullptr;
  float* ev_kin = nullptr;
  int ev_table_E = 0;
  int ev_normc_ok = 0;
  // evaluation members (ddrl_eval_members_*): mem_on = M while the mode is on, member m owns the
  // envs [m n, (m + 1) n).  Per member: the flat parameters of every policy (mem_theta[p], stride
  // mem_tstride[p] floats), the env-side filter block (FM_* layout), the per-policy filter state
  // [P][PF_STRIDE] and the chunk scratch of the filter push.  mem_cap: the M the buffers hold;
  // mem_normc_ok: every member's filter constants are current
  int mem_on = 0, mem_cap = 0, mem_normc_ok = 0;
  float* mem_theta[DDRL_MAXP] = {nullptr};
  size_t mem_tstride[DDRL_MAXP] = {0};
  double *mem_filt = nullptr, *mem_pf = nullptr, *mem_part = nullptr;
  std::vector<char> mem_loaded;
  // input sensitivity (ddrl_eval_sens_*): the steps [P][DDRL_MAXD], per policy the per-base-row
  // accumulators [C][2][d][A] and step counts [C], the reduced result; sens_act_ok: a
  // ddrl_eval_act has run since the filter constants may last have changed
  int sens_on = 0, sens_act_ok = 0;
  double* sens_step = nullptr;
  double* sens_acc[DDRL_MAXP] = {nullptr};
  long long* sens_cnt[DDRL_MAXP] = {nullptr};
  double* sens_red = nullptr;      // [2 * DDRL_MAXD * 8] + one int64
  // episode accounting (ddrl_episodes_*), allocated by the first call: the in-flight state of
  // every env (interleaved total, per-agent totals, length), the per-(step, wave) counts and
  // their scan, the table of the last collect (ep_cap rows of 8 doubles, ep_rows written);
  // ep_collected: the fragment the context holds has been walked (rewards / records re-arm it)
  double *ep_total = nullptr, *ep_agent = nullptr, *ep_table = nullptr;
  int *ep_len = nullptr, *ep_cnt = nullptr;
  long long *ep_base = nullptr, *ep_word = nullptr;
  long long ep_cap = 0, ep_rows = -1;
  int ep_collected = 0;
  // device env planes bound to this context (ddrl_devenv_*), and ddrl_rollout_devenv's graph:
  // keyed by the env's id, its settings generation and the noise buffer
  std::vector<ddrl_devenv*> devenvs;
  hipGraphExec_t rgd_exec = nullptr;
  uint64_t rgd_env = 0;
  unsigned rgd_gen = 0;
  const void* rgd_eps = nullptr;
  // device randomness (ddrl_rng_*): the noise and the schedule stream (DDRL_RNG_*), each a seed and
  // a position, all of the generator's state; unseeded streams refuse every draw
  struct RngStream { uint64_t seed = 0, pos = 0; int seeded = 0; } rng[2];
  RngTables* rng_tabs = nullptr;   // allocated by the first group fill with this context as member 0
  std::vector<void*> allocs;
};

// A device env plane (devenv.hip): the kernel arguments (state and output buffers in device
// memory), the host copy of the target-velocity list and the scratch of state_get / state_set.
struct ddrl_devenv {
  ddrl_ctx* ctx = nullptr;       // null once the context is gone
  uint64_t id = 0;               // unique per process (a graph key must not be an address that is reused)
  unsigned gen = 0;              // bumped by every setting a captured launch has baked in
  DevEnvArgs a{};
  std::vector<double> tv_list;
  double* tv_dev = nullptr;
  size_t tv_cap = 0;
  double* tv_env_dev = nullptr;   // [N] per-env velocities (set_env_target_velocities), allocated on first use
  double* packed = nullptr;
  std::vector<void*> allocs;
};

namespace ddrl_impl {
template <class T>
int dalloc(ddrl_ctx* c, T** p, size_t count) {
  void* ptr = nullptr;
  const char* step = nullptr;
  const hipError_t e = dev_zalloc(&ptr, count * sizeof(T), &step);
  if (e != hipSuccess) return fail(std::string(step) + " failed: " + hipGetErrorString(e));
  c->allocs.push_back(ptr);
  *p = static_cast<T*>(ptr);
  return 0;
}

// a buffer that is replaced by a larger one (the data-parallel loop's chunk and slots): the
// callers run after a stream synchronize, so nothing in flight still reads it
template <class T>
void dfree(ddrl_ctx* c, T** p) {
  if (!*p) return;
  auto it = std::find(c->allocs.begin(), c->allocs.end(), static_cast<void*>(*p));
  if (it != c->allocs.end()) c->allocs.erase(it);
  (void)hipFree(*p);
  *p = nullptr;
}

// Grow *p to hold `need` units of `per` elements when *cap counts fewer: a new zeroed buffer, the old contents are
// gone (*cap is 0 while there is none).  The caller has made sure that nothing in flight reads the old one.
template <class T, class N>
int dgrow(ddrl_ctx* c, T** p, N* cap, size_t need, size_t per = 1) {
  if ((size_t)*cap >= need) return 0;
  dfree(c, p);
  *cap = 0;
  if (dalloc(c, p, need * per)) return -1;
  *cap = (N)need;
  return 0;
}

// "cup" model: the leg-coupling table [4][A] follows the policy's fcnet variables (null: none)
inline const float* cup_table(const ddrl_ctx* c, int p) {
  return c->cfg.leg_coupling ? c->pol[p].theta + ffn_param_count(c->pol[p].d, c->cfg.act_dim) : nullptr;
}

// the clip of the env-side filter as the kernels take it (0: none)
inline float effective_clip(const ddrl_cfg& g) { return g.filter_enabled ? g.filter_clip : 0.f; }

// stream-ordered copy of a host env plane's pinned buffer
inline int h2d(ddrl_ctx* c, void* dst, const void* src, size_t bytes) {
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream) == hipSuccess ? 0 : fail("H2D copy failed");
}

// the steps a launch runs of a schedule of `total`, from step0, at most max_steps of them (< 0: all that are left)
inline int steps_to_run(int total, int step0, int max_steps) {
  return max_steps >= 0 ? std::min(total - step0, max_steps) : total - step0;
}

// ---- the helpers that cross files, under the file that defines them ----
// capi_ctx.cpp
int snapshot(ddrl_ctx* c, int mask);
int restore_snapshot(ddrl_ctx* c);
void peer_detach(ddrl_ctx* c);
int check_err(ddrl_ctx* c);
// capi_rollout.cpp
RewardArgs make_reward(ddrl_ctx* c);
int graph_run(ddrl_ctx* c, hipGraphExec_t* exec, bool stale, const std::function<int()>& launches);
void rollout_ran(ddrl_ctx* c);
int ep_state(ddrl_ctx* c);                        // the episode accounting's buffers, allocated on first use
int ep_table_fit(ddrl_ctx* c, long long total);   // count check + table growth of a collect
// capi_devenv.cpp
int chk_env_of(const ddrl_ctx* c, const ddrl_devenv* e);
// capi_update.cpp
UpdateHyper make_hyper(ddrl_ctx* c, int P);
UpdateArgs make_update(ddrl_ctx* c, int p, const int32_t* shuffle, const int32_t* perm, float kl);
// capi_group.cpp (`kind` names the group in the messages: "update", "rollout", "noise fill", ...)
std::string group_member_name(const char* kind, int m);
int group_list_ok(const char* kind, ddrl_ctx* const* members, ddrl_devenv* const* envs, int n_members);
int group_same_result(const char* kind, int m, const char* why);
}  // namespace ddrl_impl

