// Counter-based randomness of the device generator (rng.hip): Philox4x32-10, the standard normals
// of the exploration noise and the keyed permutations of the minibatch schedules.  Every draw is a
// pure function of (seed, position, element): no state in device memory, no ordering between
// lanes.  The layouts below are the ones DESIGN.md section 3 "Device randomness" states; the test
// oracle (tests/rng_oracle.py) is a numpy restatement of that text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace philox {

struct u32x4 { uint32_t x, y, z, w; };

constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;   // Random123's multipliers
constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;   // ... and key increments

// Philox4x32-10: ten rounds, the key bumped between them (nine times)
__device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
    const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
    c = u32x4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += W0;
    k1 += W1;
  }
  return c;
}

// ---- exploration noise ----
// u = ((w >> 8) + 0.5) * 2^-24 in (0, 1]: the 24-bit integer is exact in fp32, the sum rounds once
__device__ __forceinline__ float unit24(uint32_t w) { return __fmaf_rn((float)(w >> 8), 0x1p-24f, 0x1p-25f); }

// Box-Muller on (w0, w1): r = sqrt(-2 ln u1), (r cos 2 pi u2, r sin 2 pi u2).  The hardware sine and
// cosine take their argument in revolutions, which is u2 itself.
__device__ __forceinline__ void box_muller(uint32_t w0, uint32_t w1, float& z0, float& z1) {
  const float r = sqrtf(-2.f * logf(unit24(w0)));
  const float u2 = unit24(w1);
  z0 = r * __builtin_amdgcn_cosf(u2);
  z1 = r * __builtin_amdgcn_sinf(u2);
}

// The four normals of block b of env e at absolute step s: components 4 b .. 4 b + 3 of the env's
// flat (agent, action) vector.  counter = (s lo, s hi, e, b), key = (seed lo, seed hi).
__device__ __forceinline__ float4 noise_block(uint64_t seed, uint64_t s, uint32_t e, uint32_t b) {
  const u32x4 w = philox4x32_10(u32x4{(uint32_t)s, (uint32_t)(s >> 32), e, b}, (uint32_t)seed, (uint32_t)(seed >> 32));
  float4 z;
  box_muller(w.x, w.y, z.x, z.y);
  box_muller(w.z, w.w, z.z, z.w);
  return z;
}

// ---- schedules ----
// Array `a` of policy p in draw d of a schedule stream is the bijection of [0, n) below; a = 0 is
// the row shuffle, a = 1 + e the minibatch-slot permutation of epoch e.
// Round function: word 0 of Philox(counter = (x, d lo, d hi, 2^31 | p << 28 | r << 24 | a), key = seed).
// Bit 31 of counter word 3 keeps these blocks apart from the noise blocks of an equal seed.
__device__ __forceinline__ uint32_t schedule_tag(int p, uint32_t a) { return 0x80000000u | ((uint32_t)p << 28) | a; }

// half width of the Feistel network: the smallest h >= 1 with 4^h >= n
__host__ __device__ __forceinline__ int feistel_half_bits(uint32_t n) {
  int h = 1;
  while (h < 16 && (1ull << (2 * h)) < n) ++h;
  return h;
}

constexpr int FEISTEL_ROUNDS = 4;

// Element i of the permutation: a balanced Feistel network of FEISTEL_ROUNDS rounds over 2 h bits,
// (L, R) <- (R, L ^ F_r(R)), walked (applied again) until the value is below n.  A bijection of
// [0, 4^h) restricted this way is a bijection of [0, n); i < n is on a cycle that returns to it, so
// the walk ends.
__device__ __forceinline__ uint32_t feistel_permute(uint64_t seed, uint64_t d, uint32_t tag, uint32_t n, int h, uint32_t i) {
  const uint32_t mask = (1u << h) - 1u;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t v = i;
  do {
    uint32_t L = v >> h, R = v & mask;
#pragma unroll
    for (uint32_t r = 0; r < (uint32_t)FEISTEL_ROUNDS; ++r) {
      const uint32_t f = philox4x32_10(u32x4{R, (uint32_t)d, (uint32_t)(d >> 32), tag | (r << 24)}, k0, k1).x;
      const uint32_t t = L ^ (f & mask);
      L = R;
      R = t;
    }
    v = (L << h) | R;
  } while (v >= n);
  return v;
}

}  // namespace philox
