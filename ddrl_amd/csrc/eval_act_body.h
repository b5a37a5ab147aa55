// The body of k_eval_act (eval.hip) and k_eval_act_members (eval_members.hip), included inside the
// kernel's braces.  Operands: ra (RouteArgs; N = the envs rows are counted in), the template arguments
// A, KS1, and EVAL(field), the unit's name at its point of use for obs, normc, pf, clip, eps, actions
// and for policy p's theta, cup and logits_out.  EVAL_TILE_GUARD: what a wave does once the weights
// are staged and the barrier is met (nothing in k_eval_act).
  constexpr int O = 2 * A;
  extern __shared__ float lds[];
  const int p = blockIdx.y;
  const PolicyRoute& pr = ra.pol[p];
  const int row_hi = ra.N * pr.k;
  const int row0 = blockIdx.x * 64;
  if (row0 >= row_hi) return;
  const int d = pr.d;
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4, w = threadIdx.x >> 6;
  const int row = row0 + 16 * w + c;
  const bool valid = row < row_hi;
  const int rv = valid ? row : 0;
  const int e = rv / pr.k, slot = rv - e * pr.k;
  const float* o = EVAL(obs) + (size_t)e * ra.full_dim;
  const double* P = policy_filter_normc(EVAL(pf), p);
  float xop[12];
#pragma unroll
  for (int s = 0; s < 12; ++s) {
    const int f = 4 * s + q;
    float v = 0.f;
    if (s < KS1 && f < d && valid) v = routed_input(pr, slot, f, o, EVAL(normc), EVAL(clip), P);
    xop[s] = v;
  }
  // the weights are staged after the operand loads were issued: the fp64 normalization runs
  // while the weight loads are in flight
  NetLds PW;
  stage_policy_weights(EVAL(theta), d, A, lds, PW, 256);
  __syncthreads();
  EVAL_TILE_GUARD
  floatx4 h1[4], h2[4];
  float logits[O];
  ffn_branch_fwd<O, KS1>(PW, xop, h1, h2, logits);
  if (!valid) return;
  const int agent = pr.agent[slot];
  // "cup" model: mean_j *= coupling[leg][j], leg = the agent's slot (k_act_ffn).  In place in each
  // kernel: through a shared helper the A = 2 instances of k_eval_act measured 0.2 us longer
  if (EVAL(cup)) {
#pragma unroll
    for (int j = 0; j < A; ++j) logits[j] *= EVAL(cup)[slot * A + j];
  }
  if (q == 0) {
#pragma unroll
    for (int j = 0; j < A; ++j) {
      const float mu = logits[j], ls = logits[A + j];
      float act = mu;   // deterministic: the DiagGaussian mean (explore=False)
      if (EVAL(eps)) {
        const float sd = expf(ls);
        const float eps = EVAL(eps)[((size_t)e * ra.n_agents + agent) * A + j];
        act = mu + sd * eps;
      }
      scatter_action(EVAL(actions), pr, e, slot, j, act);
    }
  } else if (q == 1 && EVAL(logits_out)) {
    float* lo = EVAL(logits_out) + (size_t)row * O;
#pragma unroll
    for (int j = 0; j < O; ++j) lo[j] = logits[j];
  }
#undef EVAL
#undef EVAL_TILE_GUARD
