// The QuAntruped stand-in's dynamics, once, for both env planes: the host plane (hostenv.cpp,
// a thread pool over these functions) and the device plane (devenv.hip, kernels over the same
// functions).  See hostenv.h for what the stand-in is and is not.
//
// Arithmetic contract: every expression below is IEEE fp64 / fp32 or integer arithmetic in a
// fixed order, so the two planes agree bit for bit wherever no sin / cos result enters -- the
// translation units that include this header must not contract a * b + c into an fma (the host
// build targets baseline x86-64, which has none; devenv.hip turns contraction off).  sin / cos
// are the platform's fp64 library functions (glibc on the host, the device library on the GPU)
// and may differ in the last places.  min / max / fabs are spelled out (dmin, dmax, dabs) with
// the operand order of std::min / std::max, so a NaN takes the same way on both planes.
//
// The step is split into the pieces a kernel with one lane per leg needs (leg_contact,
// accum_leg, joint_step, torso_step, ...); step_env composes them for one thread per env.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ENVDYN_HD __host__ __device__ inline

namespace envdyn {

struct EnvState {
  double x, y, z, vx, vy, vz;       // torso position / velocity
  double roll, pitch, wroll, wpitch;
  double q[8], qd[8];               // joints: [FL hip, FL knee, HL hip, HL knee, HR hip, HR knee, FR hip, FR knee]
  double qfrc[8];                   // last actuator + constraint force per joint
  double foot[4];                   // last contact force per foot
  int steps;                        // steps in the current episode
  uint32_t episode;
  double tv;                        // target velocity of the current episode (TVel envs)
};

// The packed state of one env as the state_get / state_set calls of both planes exchange it
// (DDRL_ENV_STATE_DOUBLES of include/ddrl_hip.h): torso {x, y, z, vx, vy, vz, roll, pitch, wroll,
// wpitch}, q[8], qd[8], qfrc[8], foot[4], steps, episode, tv.
constexpr int kStateDoubles = 41;

constexpr double kH = 0.01;           // integration step; frame_skip 5 -> 0.05 s per env step
constexpr int kFrameSkip = 5;
constexpr double kDt = kH * kFrameSkip;
constexpr double kGear = 30.0, kSpring = 8.0, kDamp = 1.5, kLimit = 1.4;
constexpr double kShin = 0.7, kHipOff = 0.08, kGround = 400.0, kGroundDamp = 8.0;
constexpr uint64_t kTvDraw = 1u << 20;   // counter index of the target-velocity draw (pose draws use 0..16)

// rest pose (knees bent): {0, 1, 0, -1, 0, -1, 0, 1}
ENVDYN_HD double q_rest(int j) { return (j & 1) == 0 ? 0.0 : ((j == 1 || j == 7) ? 1.0 : -1.0); }

ENVDYN_HD double dmin(double a, double b) { return b < a ? b : a; }   // std::min(a, b)
ENVDYN_HD double dmax(double a, double b) { return a < b ? b : a; }   // std::max(a, b)
ENVDYN_HD double dabs(double a) { return __builtin_fabs(a); }

// counter-based generator: uniform in [-1, 1) from (seed, env, episode, draw)
ENVDYN_HD double hash_uniform(uint64_t seed, uint64_t env, uint64_t episode, uint64_t k) {
  uint64_t z = seed ^ (env * 0x9E3779B97F4A7C15ull) ^ (episode * 0xBF58476D1CE4E5B9ull) ^ (k * 0x94D049BB133111EBull);
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// the same hash in two halves, for callers that draw many values under one (seed, env, episode):
// hash_draw(hash_key(seed, env, episode), k) == hash_uniform(seed, env, episode, k) bit for bit
ENVDYN_HD uint64_t hash_key(uint64_t seed, uint64_t env, uint64_t episode) {
  return seed ^ (env * 0x9E3779B97F4A7C15ull) ^ (episode * 0xBF58476D1CE4E5B9ull);
}
ENVDYN_HD double hash_draw(uint64_t key, uint64_t k) {
  uint64_t z = key ^ (k * 0x94D049BB133111EBull);
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// ---- terrain: a procedural height field, a pure function of (seed, env, generation, episode,
// smoothness bounds, x, y) -- no stored height map (the reference's create_new_hfield,
// quantruped_v3.py:25-54, draws uniform(smoothness, 1) on a coarse grid, upsamples it, subtracts
// the minimum and clears a start patch).
//
//   settings   lo <= hi in [0, 1] (1: flat), bump_scale (m), generation; inv_bump = 1.0 / bump_scale
//              is formed once on the host, by the same division on both planes
//   smoothness of env e in generation g:  s = hi - us * (hi - lo),
//              us = 0.5 * (hash_uniform(seed ^ kSmoothSalt, e, g, 0) + 1.0)  in [0, 1)
//   field id   G = (generation << 32) | episode: every episode of an env walks on new ground (the
//              reference makes a new field before every evaluation episode), and new_terrain
//              (generation += 1) renews the ground of every env
//   cell       gx = clamp(x * inv_bump, -kCellMax, kCellMax), fi = floor(gx), tx = gx - fi, likewise y;
//              lattice value u(i, j) = 0.5 * (hash_uniform(seed ^ kTerrainSalt, e, G,
//              (uint32(i) << 32) | uint32(j)) + 1.0)  in [0, 1)
//   weights    wx = tx * tx * (3.0 - 2.0 * tx), wy likewise (smoothstep: the field is continuous
//              across cell boundaries and so is its gradient)
//   interp     a0 = u00 + wx * (u10 - u00);  a1 = u01 + wx * (u11 - u01);  U = a0 + wy * (a1 - a0)
//              (u_ab: the value at cell (i + a, j + b)); U stays in [0, 1] in fp64 as well
//   ramp       r = max(|x|, |y|); tr = clamp((r - 0.8) * 0.625, 0, 1); ramp = tr * tr * (3.0 - 2.0 * tr):
//              exactly 0.0 on the start patch r <= 0.8, 1.0 from r = 2.4 on
//   height     h = ((1.0 - s) * kElevation) * U * ramp  in [0, 1 - s]
// The reference's lattice value is s + (1 - s) * u and its height (interp - s) * elevation; the
// common factor (1 - s) is taken out of the interpolation here, which is the same function, makes
// s = 1 exactly 0.0 and keeps the bounds exact.  Only floor, + - *, comparisons and integer
// arithmetic: the two planes agree on h bit for bit.
struct Terrain {
  double lo, hi, bump_scale, inv_bump;
  uint32_t generation;
};
ENVDYN_HD Terrain terrain_flat() { return Terrain{1.0, 1.0, 2.0, 1.0 / 2.0, 0u}; }
// flat ground runs the step without any of this (the same expressions as before terrain existed)
ENVDYN_HD bool terrain_on(const Terrain& t) { return !(t.lo == 1.0 && t.hi == 1.0); }

constexpr uint64_t kTerrainSalt = 0x7E44A1F0C0DE5EEDull, kSmoothSalt = 0x5300074E55D4A3B1ull;
constexpr double kElevation = 1.0;            // the reference's hfield z size
constexpr double kPatch = 0.8, kPatchRim = 0.625;   // cleared start patch; 1 / 1.6, the width of its rim (exact)
constexpr double kCellMax = 1073741824.0;     // 2^30 cells either way: the cell index fits an int32

// the ground of one env for one step: what does not depend on the point
struct Ground {
  uint64_t key;      // hash_key of the field
  double amp;        // (1 - s) * kElevation
  double inv_bump;
};
ENVDYN_HD double terrain_smoothness(const Terrain& t, uint64_t seed, int e) {
  const double us = 0.5 * (hash_uniform(seed ^ kSmoothSalt, e, t.generation, 0) + 1.0);
  return t.hi - us * (t.hi - t.lo);
}
ENVDYN_HD Ground ground_of(const Terrain& t, uint64_t seed, int e, uint32_t episode) {
  const uint64_t G = ((uint64_t)t.generation << 32) | (uint64_t)episode;
  return Ground{hash_key(seed ^ kTerrainSalt, e, G), (1.0 - terrain_smoothness(t, seed, e)) * kElevation, t.inv_bump};
}
ENVDYN_HD double smoothstep01(double t) { return t * t * (3.0 - 2.0 * t); }
ENVDYN_HD double ground_height(const Ground& g, double x, double y) {
  const double gx = dmax(-kCellMax, dmin(kCellMax, x * g.inv_bump));
  const double gy = dmax(-kCellMax, dmin(kCellMax, y * g.inv_bump));
  const double fi = __builtin_floor(gx), fj = __builtin_floor(gy);
  const double wx = smoothstep01(gx - fi), wy = smoothstep01(gy - fj);
  const uint32_t i = (uint32_t)(int32_t)fi, j = (uint32_t)(int32_t)fj;
  const uint64_t i0 = (uint64_t)i << 32, i1 = (uint64_t)(i + 1u) << 32;
  const uint64_t j0 = j, j1 = j + 1u;
  const double u00 = 0.5 * (hash_draw(g.key, i0 | j0) + 1.0), u10 = 0.5 * (hash_draw(g.key, i1 | j0) + 1.0);
  const double u01 = 0.5 * (hash_draw(g.key, i0 | j1) + 1.0), u11 = 0.5 * (hash_draw(g.key, i1 | j1) + 1.0);
  const double a0 = u00 + wx * (u10 - u00);
  const double a1 = u01 + wx * (u11 - u01);
  const double U = a0 + wy * (a1 - a0);
  const double r = dmax(dabs(x), dabs(y));
  const double ramp = smoothstep01(dmax(0.0, dmin(1.0, (r - kPatch) * kPatchRim)));
  return g.amp * U * ramp;
}

// random.choice(target_velocity_list): every list position equally likely (a repeated value
// counts once per position); draw index kTvDraw of the episode's counter stream
ENVDYN_HD double draw_tv(uint64_t seed, int e, uint32_t ep, const double* tv_list, int n_tv) {
  const double u = 0.5 * (hash_uniform(seed, e, ep, kTvDraw) + 1.0);   // [0, 1)
  const size_t n = (size_t)n_tv;
  const size_t i = (size_t)(u * (double)n);
  return tv_list[n - 1 < i ? n - 1 : i];
}

// the pose draws of a fresh episode: torso height (draw 0), joint j's angle and velocity
// (draws 1 + 2j and 2 + 2j)
ENVDYN_HD double reset_z(uint64_t seed, int e, uint32_t ep) { return 0.57 + 0.01 * hash_uniform(seed, e, ep, 0); }
ENVDYN_HD double reset_q(uint64_t seed, int e, uint32_t ep, int j) {
  return q_rest(j) + 0.1 * hash_uniform(seed, e, ep, 1 + 2 * j);
}
ENVDYN_HD double reset_qd(uint64_t seed, int e, uint32_t ep, int j) {
  return 0.1 * hash_uniform(seed, e, ep, 2 + 2 * j);
}

// a fresh episode of env e: new initial pose and, when draw, a new target velocity
ENVDYN_HD void reset_env(EnvState& s, uint64_t seed, int e, bool draw, const double* tv_list, int n_tv) {
  const uint32_t ep = s.episode + 1;
  const double tv = s.tv;
  s = EnvState{};
  s.episode = ep;
  s.tv = draw ? draw_tv(seed, e, ep, tv_list, n_tv) : tv;
  s.z = reset_z(seed, e, ep);
  for (int j = 0; j < 8; ++j) {
    s.q[j] = reset_q(seed, e, ep, j);
    s.qd[j] = reset_qd(seed, e, ep, j);
  }
}

// staggered episode phases of a full reset, like a long-running sampler
ENVDYN_HD int stagger_steps(uint64_t seed, int e, int time_limit) {
  return (int)(((uint64_t)e * 2654435761ull + seed) % (uint64_t)time_limit);
}

// quaternion (w, x, y, z) of roll about x then pitch about y
ENVDYN_HD void quat_of(double cr, double sr, double cp, double sp, double w[4]) {
  w[0] = cr * cp; w[1] = sr * cp; w[2] = cr * sp; w[3] = -sr * sp;
}
ENVDYN_HD void quat(double roll, double pitch, double w[4]) {
  quat_of(cos(0.5 * roll), sin(0.5 * roll), cos(0.5 * pitch), sin(0.5 * pitch), w);
}

// obs columns: [0] z, [1..4] quaternion, [5..12] joint angles, [13..18] torso velocities
// (vx, vy, vz, wroll, wpitch, 0), [19..26] joint velocities, [27..34] forces, [35..42] ctrl,
// [43] target velocity (D = 44)
constexpr int kObsQ = 5, kObsVel = 13, kObsQd = 19, kObsFrc = 27, kObsCtrl = 35, kObsTv = 43;

ENVDYN_HD void write_obs(const EnvState& s, float* o, int D, const double* ctrl) {
  double w[4];
  quat(s.roll, s.pitch, w);
  o[0] = (float)s.z;
  for (int i = 0; i < 4; ++i) o[1 + i] = (float)w[i];
  for (int j = 0; j < 8; ++j) o[kObsQ + j] = (float)s.q[j];
  o[kObsVel + 0] = (float)s.vx; o[kObsVel + 1] = (float)s.vy; o[kObsVel + 2] = (float)s.vz;
  o[kObsVel + 3] = (float)s.wroll; o[kObsVel + 4] = (float)s.wpitch; o[kObsVel + 5] = (float)0.0;
  for (int j = 0; j < 8; ++j) o[kObsQd + j] = (float)s.qd[j];
  for (int j = 0; j < 8; ++j) o[kObsFrc + j] = (float)s.qfrc[j];
  for (int j = 0; j < 8; ++j) o[kObsCtrl + j] = (float)(ctrl ? ctrl[j] : 0.0);
  if (D > 43) o[kObsTv] = (float)s.tv;
}

ENVDYN_HD double clip_action(float a) { return dmin(1.0, dmax(-1.0, (double)a)); }

// one leg of one substep: the contact force of its foot and its push on the torso.  Foot height
// below the hip: shin along the knee angle, hip swing lifts it a little; a stance foot pushes
// the torso by the hip's backward swing.
ENVDYN_HD void leg_contact(double z, double vz, double q_hip, double q_knee, double qd_hip, double& force,
                           double& push) {
  const double fz = z - kShin * cos(q_knee) * cos(q_hip) + kHipOff * dabs(sin(q_hip));
  force = 0.0;
  if (fz < 0.0) force = dmax(0.0, -kGround * fz - kGroundDamp * vz);
  push = force * 0.05 * (-qd_hip) * cos(q_hip);
}

// leg_contact on uneven ground: the foot's ground height is the field under the foot's world
// position -- the torso's (x, y), the leg's fixed offset (front / side signs as in accum_leg) and
// the hip swing's x displacement of the shin -- and the flat expression's fz is lowered by it.
// The joints do not feel the ground (joint_step reads no force), unhealthy() keeps the absolute
// height test and the thrust has no slope term, as on flat ground.
// The leg's offset from the torso's centre: the Ant's foot tips at rest, 0.8 m out in x and in y
// (hip at 0.2, upper leg to 0.4, lower leg to 0.8).  A fresh episode so starts with the torso on
// the cleared patch and the feet on its edge: a leg that swings outwards steps onto rising ground.
constexpr double kFootDX = 0.8, kFootDY = 0.8;
ENVDYN_HD void leg_contact_on(const Ground& g, int leg, double x, double y, double z, double vz, double q_hip,
                              double q_knee, double qd_hip, double& force, double& push) {
  const double ck = cos(q_knee), sh = sin(q_hip), ch = cos(q_hip);
  const double side = (leg == 0 || leg == 1) ? 1.0 : -1.0;
  const double front = (leg == 0 || leg == 3) ? 1.0 : -1.0;
  const double h = ground_height(g, x + front * kFootDX + kShin * ck * sh, y + side * kFootDY);
  const double fz = z - kShin * ck * ch + kHipOff * dabs(sh) - h;
  force = 0.0;
  if (fz < 0.0) force = dmax(0.0, -kGround * fz - kGroundDamp * vz);
  push = force * 0.05 * (-qd_hip) * ch;
}

// the four per-leg terms summed over the legs in the order 0, 1, 2, 3 from 0.0
struct LegSums {
  double thrust, lift, troll, tpitch;
};
ENVDYN_HD LegSums leg_sums_zero() { return LegSums{0.0, 0.0, 0.0, 0.0}; }
ENVDYN_HD void accum_leg(LegSums& a, int leg, double force, double push) {
  a.thrust += push;
  a.lift += force;
  const double side = (leg == 0 || leg == 1) ? 1.0 : -1.0;    // FL, HL left; HR, FR right
  const double front = (leg == 0 || leg == 3) ? 1.0 : -1.0;   // FL, FR front
  a.troll += side * force;
  a.tpitch += front * force;
}

// one joint of one substep (a: the clipped action)
ENVDYN_HD void joint_step(int j, double a, double& q, double& qd, double& qfrc) {
  const double tau = kGear * a;
  double qdd = tau - kSpring * (q - q_rest(j)) - kDamp * qd;
  qd += kH * qdd;
  q += kH * qd;
  double constraint = 0.0;
  if (q > kLimit || q < -kLimit) {   // joint limit: stop and report the reaction
    const double lim = q > 0 ? kLimit : -kLimit;
    constraint = -(q - lim) / (kH * kH);
    q = lim;
    qd = 0.0;
  }
  qfrc = tau + dmax(-100.0, dmin(100.0, constraint));
}

// the torso of one substep
struct Torso {
  double x, y, z, vx, vy, vz, roll, pitch, wroll, wpitch;
};
ENVDYN_HD void torso_step(Torso& s, const LegSums& a) {
  s.vx += kH * (a.thrust - 0.8 * s.vx);
  s.vy += kH * (-0.8 * s.vy + 0.02 * a.troll * sin(s.roll));
  s.vz += kH * (a.lift / 8.0 - 9.81 - 1.0 * s.vz);
  s.wroll += kH * (0.02 * a.troll - 4.0 * s.roll - 1.5 * s.wroll);
  s.wpitch += kH * (0.02 * a.tpitch - 4.0 * s.pitch - 1.5 * s.wpitch);
  s.x += kH * s.vx;
  s.y += kH * s.vy;
  s.z += kH * s.vz;
  s.roll += kH * s.wroll;
  s.pitch += kH * s.wpitch;
}

// forward reward of the step (quantruped_v3.py:163-179): the torso's x velocity; the TVel
// envs reward reaching the target velocity instead (QuAntrupedTVelEnv.compute_forward_reward,
// quantruped_v3.py:391-392)
ENVDYN_HD float forward_reward(double x, double x0, double tv, int D) {
  const double vx = (x - x0) / kDt;
  if (D > 43) return (float)((1.0 + 1.0 / tv) * (1.0 / (dabs(vx - tv) + 1.0) - 1.0 / (tv + 1.0)));
  return (float)vx;
}

// cfrc_ext [14][6]: {floor, torso, then hip / leg / foot of FL, HL, HR, FR}; rotational then
// linear part, the contact force on the foot bodies.  The foot body's row {r0, 0, 0, r3, 0, r5},
// and the leg's fp32 share of the torso row's last column (summed in leg order)
ENVDYN_HD void foot_row(double f, double q_hip, float& r0, float& r3, float& r5) {
  r0 = (float)(0.01 * f * sin(q_hip));
  r3 = (float)(0.1 * f * sin(q_hip));
  r5 = (float)f;
}
ENVDYN_HD float torso_share(double f) { return (float)(0.05 * f); }

ENVDYN_HD bool unhealthy(double z) { return !(z > 0.1 && z < 1.5) || !__builtin_isfinite(z); }

// One env step for one thread: the actions a8[8] into the state and the env's outputs
// (obs [D], fw, cfrc [14][6], kin [9] = {dx, qd[0..7]} before a done env is reset, done).
// terrain: null on flat ground (the flat leg_contact), else the settings of an uneven field.
ENVDYN_HD void step_env(EnvState& s, const float* a8, float* obs, float* fw, float* cf, float* kn, uint8_t* done,
                        int D, int time_limit, uint64_t seed, int e, const double* tv_list, int n_tv,
                        const Terrain* terrain = nullptr) {
  const Ground g = terrain ? ground_of(*terrain, seed, e, s.episode) : Ground{0, 0.0, 0.0};
  double a[8];
  for (int j = 0; j < 8; ++j) a[j] = clip_action(a8[j]);
  const double x0 = s.x;
  Torso t{s.x, s.y, s.z, s.vx, s.vy, s.vz, s.roll, s.pitch, s.wroll, s.wpitch};
  for (int f = 0; f < kFrameSkip; ++f) {
    LegSums sums = leg_sums_zero();
    for (int leg = 0; leg < 4; ++leg) {
      const int hip = 2 * leg, knee = hip + 1;
      double force, push;
      if (terrain) leg_contact_on(g, leg, t.x, t.y, t.z, t.vz, s.q[hip], s.q[knee], s.qd[hip], force, push);
      else leg_contact(t.z, t.vz, s.q[hip], s.q[knee], s.qd[hip], force, push);
      s.foot[leg] = force;
      accum_leg(sums, leg, force, push);
    }
    for (int j = 0; j < 8; ++j) joint_step(j, a[j], s.q[j], s.qd[j], s.qfrc[j]);
    torso_step(t, sums);
  }
  s.x = t.x; s.y = t.y; s.z = t.z; s.vx = t.vx; s.vy = t.vy; s.vz = t.vz;
  s.roll = t.roll; s.pitch = t.pitch; s.wroll = t.wroll; s.wpitch = t.wpitch;
  ++s.steps;
  *fw = forward_reward(s.x, x0, s.tv, D);
  for (int i = 0; i < 14 * 6; ++i) cf[i] = 0.f;
  for (int leg = 0; leg < 4; ++leg) {
    float* foot = cf + (4 + 3 * leg) * 6;
    foot_row(s.foot[leg], s.q[2 * leg], foot[0], foot[3], foot[5]);
    cf[1 * 6 + 5] += torso_share(s.foot[leg]);
  }
  kn[0] = (float)(s.x - x0);
  for (int j = 0; j < 8; ++j) kn[1 + j] = (float)s.qd[j];
  const bool d = unhealthy(s.z) || s.steps >= time_limit;
  *done = d ? 1 : 0;
  if (d) {
    reset_env(s, seed, e, true, tv_list, n_tv);
    write_obs(s, obs, D, nullptr);
  } else {
    write_obs(s, obs, D, a);
  }
}

// packed state <-> EnvState (kStateDoubles doubles per env)
ENVDYN_HD void pack_state(const EnvState& s, double* p) {
  p[0] = s.x; p[1] = s.y; p[2] = s.z; p[3] = s.vx; p[4] = s.vy; p[5] = s.vz;
  p[6] = s.roll; p[7] = s.pitch; p[8] = s.wroll; p[9] = s.wpitch;
  for (int j = 0; j < 8; ++j) { p[10 + j] = s.q[j]; p[18 + j] = s.qd[j]; p[26 + j] = s.qfrc[j]; }
  for (int l = 0; l < 4; ++l) p[34 + l] = s.foot[l];
  p[38] = (double)s.steps; p[39] = (double)s.episode; p[40] = s.tv;
}
ENVDYN_HD void unpack_state(const double* p, EnvState& s) {
  s.x = p[0]; s.y = p[1]; s.z = p[2]; s.vx = p[3]; s.vy = p[4]; s.vz = p[5];
  s.roll = p[6]; s.pitch = p[7]; s.wroll = p[8]; s.wpitch = p[9];
  for (int j = 0; j < 8; ++j) { s.q[j] = p[10 + j]; s.qd[j] = p[18 + j]; s.qfrc[j] = p[26 + j]; }
  for (int l = 0; l < 4; ++l) s.foot[l] = p[34 + l];
  s.steps = (int)p[38]; s.episode = (uint32_t)p[39]; s.tv = p[40];
}
// steps and episode of a packed state must be integers the state's fields hold
ENVDYN_HD bool packed_counts_ok(const double* p) {
  return p[38] >= 0.0 && p[38] <= 2147483647.0 && p[38] == (double)(int)p[38] && p[39] >= 0.0 &&
         p[39] <= 4294967295.0 && p[39] == (double)(uint32_t)p[39];
}

}  // namespace envdyn
