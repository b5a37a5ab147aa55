// How far do last-place differences of sin / cos move the stand-in env?  A host-only experiment
// behind the bars of tests/test_gpu_devenv.py and tests/test_gpu_terrain.py: the dynamics of
// csrc/envdyn.h run once as they are and then with every sin / cos result moved by -1 / 0 / +1 ulp
// (a hash of a call counter decides), and the largest movement of the fp64 torso state and foot
// forces, max |nudged - plain| / (1 + |plain|), is printed with the number of done-flag and
// contact-pattern mismatches (a contact force switches on discontinuously at touch-down: a
// mismatch there makes a run useless as a yardstick, and says so).
//
//   hipcc -O2 -std=c++17 -ffp-contract=off -I include tools/envdyn_nudge.cpp -o envdyn_nudge
//   ./envdyn_nudge [smoothness=0.6] [n_envs=65] [steps=64] [seed=43] [time_limit=1000] [runs=16]
//
// Inputs, as tests/test_gpu_terrain.py's free-running parity: a full reset (staggered phases), the
// envs then placed at x = 10 m, y = -3 .. 3 m, the actions float(hash_uniform(seed, env, t, j)),
// D = 43 and D = 44 (target velocities {0.5, 1, 2}).  smoothness 1 runs the flat step.
#include <hip/hip_runtime.h>   // before sin / cos become macros

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace nudge {
static bool on = false;
static uint64_t run = 0, calls = 0;
static double apply(double v) {
  if (!on) return v;
  uint64_t z = (run * 0x9E3779B97F4A7C15ull) ^ (++calls * 0xBF58476D1CE4E5B9ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const int k = (int)(z % 3) - 1;
  return k == 0 ? v : std::nextafter(v, k > 0 ? INFINITY : -INFINITY);
}
static double nsin(double x) { return apply(std::sin(x)); }
static double ncos(double x) { return apply(std::cos(x)); }
}  // namespace nudge

#define sin(x) nudge::nsin(x)
#define cos(x) nudge::ncos(x)
#include "../ddrl_amd/csrc/envdyn.h"
#undef sin
#undef cos

using namespace envdyn;

struct Trace {
  std::vector<double> v;         // [steps][n][14]: torso 10, foot 4
  std::vector<uint8_t> done;     // [steps][n]
};

static Trace run_once(int D, double smooth, int n, int steps, uint64_t seed, int limit) {
  const double tvs[3] = {0.5, 1.0, 2.0};
  const double* tv_list = tvs;
  const int n_tv = D > 43 ? 3 : 1;
  const double zero = 0.0;
  if (D == 43) tv_list = &zero;
  Terrain ter = terrain_flat();
  ter.lo = ter.hi = smooth;
  std::vector<EnvState> st(n, EnvState{});
  for (int e = 0; e < n; ++e) {
    st[e].tv = tv_list[0];
    st[e].episode = 0;
    reset_env(st[e], seed, e, true, tv_list, n_tv);
    st[e].steps = stagger_steps(seed, e, limit);
    st[e].x = 10.0;
    st[e].y = -3.0 + 6.0 * e / (n - 1);
  }
  Trace tr;
  std::vector<float> obs(48), cf(84), kn(9);
  for (int t = 0; t < steps; ++t) {
    for (int e = 0; e < n; ++e) {
      float a8[8], fw;
      uint8_t d;
      for (int j = 0; j < 8; ++j) a8[j] = (float)hash_uniform(seed, e, t, j);
      step_env(st[e], a8, obs.data(), &fw, cf.data(), kn.data(), &d, D, limit, seed, e, tv_list, n_tv,
               terrain_on(ter) ? &ter : nullptr);
      double p[kStateDoubles];
      pack_state(st[e], p);
      for (int i = 0; i < 10; ++i) tr.v.push_back(p[i]);
      for (int i = 0; i < 4; ++i) tr.v.push_back(p[34 + i]);
      tr.done.push_back(d);
    }
  }
  return tr;
}

int main(int argc, char** argv) {
  const double smooth = argc > 1 ? atof(argv[1]) : 0.6;
  const int n = argc > 2 ? atoi(argv[2]) : 65, steps = argc > 3 ? atoi(argv[3]) : 64;
  const uint64_t seed = argc > 4 ? strtoull(argv[4], nullptr, 10) : 43;
  const int limit = argc > 5 ? atoi(argv[5]) : 1000, runs = argc > 6 ? atoi(argv[6]) : 16;
  double worst_all = 0.0;
  for (int D = 43; D <= 44; ++D) {
    nudge::on = false;
    const Trace base = run_once(D, smooth, n, steps, seed, limit);
    double worst = 0.0;
    long done_mis = 0, contact_mis = 0, ends = 0, contacts = 0;
    for (uint8_t d : base.done) ends += d;
    for (int r = 1; r <= runs; ++r) {
      nudge::on = true;
      nudge::run = r;
      nudge::calls = 0;
      const Trace tr = run_once(D, smooth, n, steps, seed, limit);
      for (size_t i = 0; i < base.done.size(); ++i) done_mis += base.done[i] != tr.done[i];
      for (size_t i = 0; i < base.v.size(); ++i) {
        if (i % 14 >= 10) {
          contact_mis += (base.v[i] > 0.0) != (tr.v[i] > 0.0);
          contacts += r == 1 && base.v[i] > 0.0;
        }
        const double err = std::fabs(tr.v[i] - base.v[i]) / (1.0 + std::fabs(base.v[i]));
        if (err > worst) worst = err;
      }
    }
    std::printf("D=%d smoothness=%g n=%d steps=%d seed=%llu limit=%d runs=%d: worst %.3e, done mismatches %ld, "
                "contact mismatches %ld (%ld episode ends, %ld foot contacts in the plain run)\n",
                D, smooth, n, steps, (unsigned long long)seed, limit, runs, worst, done_mis, contact_mis, ends, contacts);
    if (worst > worst_all) worst_all = worst;
  }
  std::printf("worst over both: %.3e\n", worst_all);
  return 0;
}
