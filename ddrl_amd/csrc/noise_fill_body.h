// The body of k_noise_fill and k_noise_fill_group (rng.hip), included inside the kernel's braces.
// Operands by name: nm (the NoiseMember: eps, seed, pos), n_steps, N, B (Philox blocks per env).
// Lane g of the flat (step, env, block) order draws block g and stores its four normals as one
// 16-byte word; the value depends on (seed, pos + step, env, block) only, not on the geometry.
  const size_t per_step = (size_t)N * B;
  const size_t total = (size_t)n_steps * per_step;
  float4* out = reinterpret_cast<float4*>(nm.eps);
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    const size_t t = g / per_step;
    const uint32_t r = (uint32_t)(g - t * per_step);
    const uint32_t e = r / (uint32_t)B;
    out[g] = philox::noise_block(nm.seed, nm.pos + t, e, r - e * (uint32_t)B);
  }
