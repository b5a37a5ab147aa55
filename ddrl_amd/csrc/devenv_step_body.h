// The body of the env-step kernel, one text for k_devenv_step (devenv.hip) and k_devenv_step_group
// (rollout_group.hip).  Included inside the kernel's braces, below `#pragma clang fp contract(off)`;
// the unit names the operands: A (DevEnvArgs), actions ([N][8]), and the template flags kTerrain, kTvEnv.
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
  const double a_h = envdyn::clip_action(actions[(size_t)e * 8 + hip]);   // envdyn::, policy_io.h has an fp32 one
  const double a_k = envdyn::clip_action(actions[(size_t)e * 8 + knee]);
  const double x0 = t.x;
  double force = 0.0, f0 = 0.0, f1 = 0.0, f2 = 0.0, f3 = 0.0;
  Ground ground{0, 0.0, 0.0};
  if constexpr (kTerrain) ground = ground_of(terrain_of(A), A.seed, e, episode);
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

  // outputs of the step, before a done env is reset.  cfrc [14][6]: lane `leg` writes the three
  // body rows of its leg (hip, leg: zero; foot), and three of the twelve floats of the floor and
  // torso rows; the torso row's last column, the fp32 sum over the legs in leg order, is lane 3's
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

  // a done env starts its next episode at once: every lane redraws the torso (the same bits),
  // its own two joints and the target velocity
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
