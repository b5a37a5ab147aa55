// The body of k_act_ffn (rollout.hip) and k_act_ffn_group (rollout_group.hip), included inside the
// kernel's braces.  Operands: ra (RouteArgs), the template arguments A, KS1, and ACT(field), the unit's
// name for a field of ActArgs at its point of use (bound to locals they cost k_act_ffn registers).
  constexpr int O = 2 * A;
  extern __shared__ float lds[];
  const int p = blockIdx.y;
  const PolicyRoute& pr = ra.pol[p];
  const int C = ACT(C)[p];
  const int row_hi = ACT(e1) * pr.k;        // rows of the env range [e0, e1)
  const int row0 = ACT(e0) * pr.k + blockIdx.x * 64;
  if (row0 >= row_hi) return;
  const int d = pr.d;
  NetLds PW, VW;
  stage_weights(ACT(theta)[p], d, A, lds, PW, VW, 512);
  __syncthreads();

  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4, w = threadIdx.x >> 6;
  const bool value_wave = w >= 4;
  if (ACT(bootstrap) && !value_wave) return;   // bootstrap: V(s_T) only
  const int row = row0 + 16 * (w & 3) + c;
  const bool valid = row < row_hi;
  const float* xs = ACT(stage)[p] + (size_t)(valid ? row : 0) * d;
  float xop[12];
#pragma unroll
  for (int s = 0; s < 12; ++s) {
    const int f = 4 * s + q;
    xop[s] = (s < KS1 && f < d && valid) ? xs[f] : 0.f;
  }
  floatx4 h1[4], h2[4];
  const RecLayout& L = ACT(lay)[p];
  if (value_wave) {
    float vout[1];
    ffn_branch_fwd<1, KS1>(VW, xop, h1, h2, vout);
    if (valid && q == 0) {
      if (ACT(bootstrap)) ACT(last_v)[p][row] = vout[0];
      else ACT(rec)[p][((size_t)ACT(t) * C + row) * L.stride + L.vf] = vout[0];
    }
    return;
  }
  float logits[O];
  ffn_branch_fwd<O, KS1>(PW, xop, h1, h2, logits);
  if (!valid) return;
  float* rp = ACT(rec)[p] + ((size_t)ACT(t) * C + row) * L.stride;
  const int e = row / pr.k, slot = row - e * pr.k;
  const int agent = pr.agent[slot];
  // "cup" model (coupling_net_glorot_uniform_init.py:22-30): mean_j *= coupling[leg][j], the
  // log-std half is padded with ones; leg = the agent's index in the env (one shared policy)
  if (ACT(cup)[p]) {
#pragma unroll
    for (int j = 0; j < A; ++j) logits[j] *= ACT(cup)[p][slot * A + j];
  }
  // sample + logp (DiagGaussian, RLlib 1.0): a = mean + std * eps
  float logp = -0.5f * (float)(DDRL_LOG2PI * A);
  float act[A];
#pragma unroll
  for (int j = 0; j < A; ++j) {
    const float mu = logits[j], ls = logits[A + j];
    const float sd = expf(ls);
    const float eps = ACT(eps)[((size_t)e * ra.n_agents + agent) * A + j];
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
      scatter_action(ACT(actions), pr, e, slot, j, act[j]);
    }
  } else if (q == 1) {
#pragma unroll
    for (int j = 0; j < O; ++j) rp[L.logit + j] = logits[j];
  } else if (q == 2) {
    rp[L.logp] = logp;
    if (L.cid >= 0) rp[L.cid] = (float)slot;
  }
#undef ACT
