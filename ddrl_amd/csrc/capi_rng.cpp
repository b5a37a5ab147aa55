// C-ABI of libddrl_hip.so: device randomness (rng.hip), noise and schedules drawn on the device.
// A stream is (seed, position) on the host; every launch gets both by value (solo) or through a
// member table (group), so the calls are asynchronous and a captured graph never holds a position.
#include "ctx.h"

namespace {
const char* const kRngName[2] = {"noise", "schedule"};

int rng_stream_ok(int stream) {
  if (stream != DDRL_RNG_NOISE && stream != DDRL_RNG_SCHEDULE) return fail("rng: stream must be DDRL_RNG_NOISE or DDRL_RNG_SCHEDULE");
  return 0;
}

std::string rng_unseeded(int stream) {
  return std::string("the ") + kRngName[stream] + " stream has no seed: call ddrl_rng_seed or ddrl_rng_state_set first";
}

// Philox blocks per env, or a refusal
int noise_blocks(const ddrl_ctx* c, int* B) {
  const int comps = c->cfg.n_agents * c->cfg.act_dim;
  if (comps < 4 || comps % 4)
    return fail("noise fill: n_agents * act_dim = " + std::to_string(comps) + " is not a multiple of 4 (one Philox block is four normals)");
  *B = comps / 4;
  return 0;
}

int noise_args_ok(int n_steps, const float* eps, const std::string& who) {
  if (n_steps < 1) return fail("noise fill: n_steps must be >= 1");
  if (!eps) return fail(who + "null noise buffer");
  if ((uintptr_t)eps % 16) return fail(who + "the noise buffer is not 16-byte aligned");
  return 0;
}

ScheduleShape schedule_shape(const ddrl_ctx* c, int mask) {
  ScheduleShape sh{};
  for (int p = 0; p < c->cfg.n_policies; ++p) {
    sh.R[p] = c->pol[p].R;
    sh.nb[p] = c->pol[p].nb;
    if (mask & (1 << p)) sh.pid[sh.n_pol++] = p;
  }
  sh.epochs = c->cfg.num_sgd_iter;
  return sh;
}

// the table of a group fill with room for n members: member 0's, grown behind a stream synchronize
template <class T>
int rng_table(ddrl_ctx* c0, MemberTable<T> RngTables::*tab, int RngTables::*cap, int n, MemberTable<T>** out) {
  if (!c0->rng_tabs) c0->rng_tabs = new RngTables();
  RngTables* t = c0->rng_tabs;
  if (t->*cap < n) {
    if (t->*cap) {
      HIPCHK(hipStreamSynchronize(c0->stream));   // the last fill read the old table
      (t->*tab).release();
      t->*tab = MemberTable<T>{};
      t->*cap = 0;
    }
    if (!(t->*tab).alloc(n)) {
      (t->*tab).release();
      t->*tab = MemberTable<T>{};
      return fail("group fill: allocation of the member table failed");
    }
    t->*cap = n;
  }
  *out = &(t->*tab);
  return 0;
}

// what both group fills ask of their member list; `kind` is "noise fill" or "schedule fill"
int rng_group_ok(const char* kind, ddrl_ctx* const* members, int n_members, int stream) {
  if (!members) return fail("null argument");
  if (n_members < 1) return fail(std::string(kind) + " group: at least one member is needed");
  if (n_members > 65535)
    return fail(std::string(kind) + " group: " + std::to_string(n_members) + " members exceed the grid's z extent (65535)");
  if (group_list_ok(kind, members, nullptr, n_members)) return -1;
  const ddrl_ctx* c0 = members[0];
  for (int m = 0; m < n_members; ++m) {
    const ddrl_ctx* c = members[m];
    if (c->device != c0->device) return fail(group_member_name(kind, m) + " is on another device than member 0");
    if (c->stream != c0->stream) return fail(group_member_name(kind, m) + " is on another stream than member 0");
    if (!c->rng[stream].seeded) return fail(group_member_name(kind, m) + ": " + rng_unseeded(stream));
  }
  return 0;
}
}  // namespace

extern "C" {

int ddrl_rng_seed(ddrl_ctx* c, int stream, uint64_t seed) { return ddrl_rng_state_set(c, stream, seed, 0); }

int ddrl_rng_state_set(ddrl_ctx* c, int stream, uint64_t seed, uint64_t position) {
  CHK_CTX(c);
  if (rng_stream_ok(stream)) return -1;
  c->rng[stream].seed = seed;
  c->rng[stream].pos = position;
  c->rng[stream].seeded = 1;
  return 0;
}

int ddrl_rng_state_get(ddrl_ctx* c, int stream, uint64_t* seed, uint64_t* position) {
  CHK_CTX(c);
  if (rng_stream_ok(stream)) return -1;
  if (!seed || !position) return fail("null argument");
  if (!c->rng[stream].seeded) return fail(rng_unseeded(stream));
  *seed = c->rng[stream].seed;
  *position = c->rng[stream].pos;
  return 0;
}

int ddrl_noise_fill(ddrl_ctx* c, int n_steps, float* eps_dev) {
  CHK_CTX(c);
  ddrl_ctx::RngStream& st = c->rng[DDRL_RNG_NOISE];
  int B = 0;
  if (!st.seeded) return fail(rng_unseeded(DDRL_RNG_NOISE));
  if (noise_args_ok(n_steps, eps_dev, "noise fill: ") || noise_blocks(c, &B)) return -1;
  HIPCHK(hipSetDevice(c->device));
  launch_noise_fill(c->stream, NoiseMember{eps_dev, st.seed, st.pos}, n_steps, c->cfg.n_envs, B);
  HIPCHK(hipGetLastError());
  st.pos += (uint64_t)n_steps;
  return 0;
}

int ddrl_schedule_fill(ddrl_ctx* c, int pid_mask, int32_t* const* shuffle_dev, int32_t* const* perm_dev) {
  CHK_CTX(c);
  ddrl_ctx::RngStream& st = c->rng[DDRL_RNG_SCHEDULE];
  if (!st.seeded) return fail(rng_unseeded(DDRL_RNG_SCHEDULE));
  if (!shuffle_dev || !perm_dev) return fail("schedule fill: null schedule table");
  if (pid_mask <= 0 || (pid_mask >> c->cfg.n_policies))
    return fail("schedule fill: pid_mask " + std::to_string(pid_mask) + " names no policy or one outside the context's " +
                std::to_string(c->cfg.n_policies));
  ScheduleMember sm{};
  for (int p = 0; p < c->cfg.n_policies; ++p) {
    if (!(pid_mask & (1 << p))) continue;
    if (!shuffle_dev[p] || !perm_dev[p]) return fail("schedule fill: null schedule buffer of policy " + std::to_string(p));
    sm.shuffle[p] = shuffle_dev[p];
    sm.perm[p] = perm_dev[p];
  }
  sm.seed = st.seed;
  sm.draw = st.pos;
  HIPCHK(hipSetDevice(c->device));
  launch_schedule_fill(c->stream, sm, schedule_shape(c, pid_mask));
  HIPCHK(hipGetLastError());
  st.pos += 1;
  return 0;
}

int ddrl_noise_fill_group(ddrl_ctx* const* members, int n_members, int n_steps, float* const* eps_dev) {
  const char* kind = "noise fill";
  if (rng_group_ok(kind, members, n_members, DDRL_RNG_NOISE)) return -1;
  if (!eps_dev) return fail("noise fill group: null noise buffer");
  ddrl_ctx* c0 = members[0];
  int B = 0;
  if (noise_blocks(c0, &B)) return -1;
  for (int m = 0; m < n_members; ++m) {
    const ddrl_cfg &x = members[m]->cfg, &y = c0->cfg;
    const char* why = x.n_envs != y.n_envs ? "n_envs" : x.n_agents != y.n_agents ? "n_agents" : x.act_dim != y.act_dim ? "act_dim" : nullptr;
    if (group_same_result(kind, m, why) || noise_args_ok(n_steps, eps_dev[m], group_member_name(kind, m) + ": ")) return -1;
  }
  HIPCHK(hipSetDevice(c0->device));
  MemberTable<NoiseMember>* tab = nullptr;
  NoiseMember* host = nullptr;
  if (rng_table(c0, &RngTables::noise, &RngTables::noise_cap, n_members, &tab) || tab->host(host)) return -1;
  for (int m = 0; m < n_members; ++m) {
    const ddrl_ctx::RngStream& st = members[m]->rng[DDRL_RNG_NOISE];
    host[m] = NoiseMember{eps_dev[m], st.seed, st.pos};
  }
  if (tab->upload(c0->stream, n_members)) return -1;
  launch_noise_fill_group(c0->stream, tab->dev, n_members, n_steps, c0->cfg.n_envs, B);
  HIPCHK(hipGetLastError());
  for (int m = 0; m < n_members; ++m) members[m]->rng[DDRL_RNG_NOISE].pos += (uint64_t)n_steps;
  return 0;
}

int ddrl_schedule_fill_group(ddrl_ctx* const* members, int n_members, int32_t* const* shuffle_dev,
                             int32_t* const* perm_dev) {
  const char* kind = "schedule fill";
  if (rng_group_ok(kind, members, n_members, DDRL_RNG_SCHEDULE)) return -1;
  if (!shuffle_dev || !perm_dev) return fail("schedule fill group: null schedule table");
  ddrl_ctx* c0 = members[0];
  const int P = c0->cfg.n_policies;
  for (int m = 0; m < n_members; ++m) {
    const ddrl_ctx* c = members[m];
    const char* why = c->cfg.n_policies != P ? "n_policies" : c->cfg.num_sgd_iter != c0->cfg.num_sgd_iter ? "num_sgd_iter" : nullptr;
    for (int p = 0; p < P && !why; ++p)
      if (c->pol[p].R != c0->pol[p].R || c->pol[p].nb != c0->pol[p].nb) why = "the rows or minibatches of a policy";
    if (group_same_result(kind, m, why)) return -1;
    for (int p = 0; p < P; ++p)
      if (!shuffle_dev[m * P + p] || !perm_dev[m * P + p])
        return fail(group_member_name(kind, m) + ": null schedule buffer of policy " + std::to_string(p));
  }
  HIPCHK(hipSetDevice(c0->device));
  MemberTable<ScheduleMember>* tab = nullptr;
  ScheduleMember* host = nullptr;
  if (rng_table(c0, &RngTables::sched, &RngTables::sched_cap, n_members, &tab) || tab->host(host)) return -1;
  for (int m = 0; m < n_members; ++m) {
    const ddrl_ctx::RngStream& st = members[m]->rng[DDRL_RNG_SCHEDULE];
    ScheduleMember sm{};
    for (int p = 0; p < P; ++p) {
      sm.shuffle[p] = shuffle_dev[m * P + p];
      sm.perm[p] = perm_dev[m * P + p];
    }
    sm.seed = st.seed;
    sm.draw = st.pos;
    host[m] = sm;
  }
  if (tab->upload(c0->stream, n_members)) return -1;
  launch_schedule_fill_group(c0->stream, tab->dev, n_members, schedule_shape(c0, (1 << P) - 1));
  HIPCHK(hipGetLastError());
  for (int m = 0; m < n_members; ++m) members[m]->rng[DDRL_RNG_SCHEDULE].pos += 1;
  return 0;
}

}  // extern "C"
