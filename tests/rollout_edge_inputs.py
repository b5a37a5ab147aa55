"""Seeded inputs and high-precision references of the rollout-plane boundary tests
(tests/test_gpu_rollout_edges.py, the multi-block cases of tests/test_gpu_eval.py), numpy only, so
that the CPU guards of tests/test_rollout_edge_inputs.py can check the inputs without a GPU."""
import numpy as np

CENTRAL, SHARED = "QuantrupedMultiEnv_Centralized", "QuantrupedMultiEnv_SharedDecentral"
LOCAL, GLOBALCOST = "QuantrupedMultiEnv_Local", "QuantrupedMultiEnv_FullyDecentralGlobalCost"

# (id, env, n envs, T, config) of the rollout + GAE parity cases at multi-unit env counts
ROLLOUT_EDGES = [
    # filter: 2 chunks, the second of one row (n_c = 1, M2 = 0); reward: 1028 lanes, 5 blocks, the
    # last ragged; GAE: C = 257, 5 waves in 2 groups, the second one wave with one live chain
    ("local257", LOCAL, 257, 3, None),
    ("centralized513", CENTRAL, 513, 2, None),            # 3 chunks; A = 8, d = 43
    # k = 4: C = 516, 9 waves in 3 groups; e = c / k beyond the first block
    ("shared129", SHARED, 129, 3, None),
    ("globalcost300", GLOBALCOST, 300, 2, None),          # reward mode 1 over 5 blocks
    ("local260_norm_reward", LOCAL, 260, 2, {"env_config": {"norm_reward": True}}),   # mode 2
]
ROLLOUT_SEED, PARAM_SEED = 11, 3
# Output-head scale of these cases.  The record's logp is the fp32 value of
# -0.5 sum z^2 - sum log_std - c with z = (a - mu) / std and a = fl(mu + std eps): z carries the
# rounding of a, up to ulp(a) / (2 std) per component, and two fp32 implementations whose means
# differ in the last bits round a differently.  With the heads scaled 30 x (the small-batch
# parity tests) |mu| reaches tens while std falls below 1e-2, and at these row counts the term
# exceeds the parity tolerance in a dozen rows per case (logp_rounding_bound; shown by
# tests/test_rollout_edge_inputs.py).  At 10 x it stays below a quarter of it in every row,
# while 3 actions in 10 still clip.
HEAD_SCALE = 10.0
LOGP_RTOL, LOGP_ATOL = 1e-5, 2e-5    # the parity tolerance of the record fields


def rollout_filter_prior(D, rng):
    return (1000.0, rng.normal(size=D) * 0.3, np.abs(rng.normal(size=D)) * 999.0 + 10.0)


def logp_rounding_bound(logits, act):
    """Per row: sum_j |z_j| ulp(a_j) / std_j, how far the fp32 logp of a sampled action can move
    when a = fl(mu + std eps) rounds the other way (d logp / d z_j = -z_j, z_j moves by at most
    ulp(a_j) / std_j between two roundings of a_j)."""
    A = act.shape[-1]
    mu, std = logits[..., :A].astype(np.float64), np.exp(logits[..., A:].astype(np.float64))
    z = (act.astype(np.float64) - mu) / std
    return (np.abs(z) * np.spacing(np.abs(act)).astype(np.float64) / std).sum(-1)


# (T, N) of the direct GAE cases: every branch of k_gae's two-chunk pipelined loop (one chunk /
# exactly one / one + ragged / exactly two / two + ragged / exactly three / three + ragged) and
# wave / group counts (64-chain waves, summed four at a time) with and without ragged tails.
GAE_SHAPES = [(1, 1), (15, 65), (16, 64), (17, 257), (32, 300), (33, 70), (48, 5), (49, 129)]
GAE_U = 16   # time steps per chunk of the kernel (gae.hip)


def gae_done_pattern(T, N, seed=0):
    """done [T, N] uint8: 10 % random flags, and on top of them forced columns, one class each,
    for the envs e with e % 8 = 0..5 (the columns 6, 7 mod 8 stay random):
      0: done at t = T - 1 only        1: done at t = 0 only
      2: done at t = T - 16 only (last step of the first chunk, when T >= 16)
      3: done at t = T - 17 only (first step of the second chunk, when T >= 17)
      4: done at every step            5: never done."""
    rng = np.random.default_rng(1000 * T + N + seed)
    done = (rng.random((T, N)) < 0.10).astype(np.uint8)
    for e in range(N):
        c = e % 8
        if c > 5:
            continue
        done[:, e] = 0
        if c == 0:
            done[T - 1, e] = 1
        elif c == 1:
            done[0, e] = 1
        elif c == 2 and T >= GAE_U:
            done[T - GAE_U, e] = 1
        elif c == 3 and T > GAE_U:
            done[T - GAE_U - 1, e] = 1
        elif c == 4:
            done[:, e] = 1
    return done


def gae_done_classes(done):
    """How many envs of a done pattern fall into each class gae_done_pattern forces."""
    T, N = done.shape
    d = done.astype(bool)
    cnt = d.sum(0)
    only = lambda t: int((d[t] & (cnt == 1)).sum()) if 0 <= t < T else 0
    return dict(last_only=only(T - 1), first_only=only(0), seam_hi_only=only(T - GAE_U),
                seam_lo_only=only(T - GAE_U - 1), always=int((cnt == T).sum()), never=int((cnt == 0).sum()),
                mixed=int(((cnt > 1) & (cnt < T)).sum()))


def gae_inputs(T, N, k, seed=0):
    """(rew [T, C], vf [T, C], done [T, N], last_v [C]) with C = N * k chains (chain c = e * k + slot)."""
    rng = np.random.default_rng(77 + 1000 * T + N + 7 * k + seed)
    C = N * k
    rew = (rng.normal(size=(T, C)) * 0.5).astype(np.float32)
    vf = (rng.normal(size=(T, C)) * 2.0).astype(np.float32)
    last_v = rng.normal(size=C).astype(np.float32)
    return rew, vf, gae_done_pattern(T, N, seed), last_v


# ---- env-side filter: hard columns ----------------------------------------------------
HARD_COL, CONST_COL, CONST_VAL = 7, 21, np.float32(0.75)


def hard_filter_pushes(N, D, pushes=4, seed=5):
    """[pushes][N, D] fp32 observations: synthetic_inputs-style columns, column HARD_COL with mean
    1000 and std 2e-3 (33 fp32 steps; S is the sum of squares of 2e-6 of the values), column
    CONST_COL constant."""
    rng = np.random.default_rng(seed + N)
    obs = (rng.normal(size=(pushes, N, D)) * 2 + 0.5).astype(np.float32)
    obs[:, :, HARD_COL] = (1000.0 + 2e-3 * rng.normal(size=(pushes, N))).astype(np.float32)
    obs[:, :, CONST_COL] = CONST_VAL
    return obs


def hard_filter_prior(D, kind, seed=6):
    """(n, M, S) before the pushes.  "fresh": (0, 0, 0).  "prior": n = 1000 and the parity tests'
    random statistics.  "matched": the same, with the hard column's own mean and spread, so that
    the merge keeps the cancellation.  The constant column's prior mean is its value in both."""
    if kind == "fresh":
        return 0.0, np.zeros(D), np.zeros(D)
    rng = np.random.default_rng(seed)
    M, S = rng.normal(size=D) * 0.3, np.abs(rng.normal(size=D)) * 999.0 + 10.0
    M[CONST_COL] = float(CONST_VAL)
    if kind == "matched":
        M[HARD_COL], S[HARD_COL] = 1000.0003, 999.0 * 2e-3 ** 2
    return 1000.0, M, S


def longdouble_filter_reference(prior, rows):
    """Two-pass mean and M2 of all pushed rows in np.longdouble, merged with the prior by Chan's
    formula in long double; returns (n, M, S) as long double."""
    L = np.longdouble
    x = np.asarray(rows, np.float32).reshape(-1, rows.shape[-1]).astype(L)
    n2 = L(x.shape[0])
    mean = x.sum(0) / n2
    m2 = ((x - mean) ** 2).sum(0)
    n1, M1, S1 = L(prior[0]), np.asarray(prior[1], L), np.asarray(prior[2], L)
    if n1 == 0:
        return n2, mean, m2
    n = n1 + n2
    delta = M1 - mean
    return n, (n1 * M1 + n2 * mean) / n, S1 + m2 + delta * delta * n1 * n2 / n


def relative_deviation(got, ref):
    """|got - ref| / |ref| per column in long double; 0 where both are equal (a zero reference
    included), inf where the reference is 0 and the value is not."""
    L = np.longdouble
    got, ref = np.asarray(got, L), np.asarray(ref, L)
    diff = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, L(0), diff / np.abs(ref))
    return r


def emulate_chunked_push(state, obs, rows=256):
    """k_filter_chunk / k_filter_merge in numpy fp64: per 256-row chunk the two-pass (mean, M2), the
    chunks merged in order (Chan), the batch merged into the running (n, M, S).  The order of the
    sums inside a chunk is numpy's, not the kernel's wave order."""
    n1, M, S = float(state[0]), np.array(state[1], np.float64), np.array(state[2], np.float64)
    x = np.asarray(obs, np.float32).astype(np.float64)
    N = x.shape[0]
    nb, mean_b, s_b = 0.0, np.zeros_like(M), np.zeros_like(S)
    for c0 in range(0, N, rows):
        ch = x[c0:c0 + rows]
        nc = float(ch.shape[0])
        mc = ch.sum(0) / nc
        m2 = ((ch - mc) ** 2).sum(0)
        nn, d = nb + nc, mc - mean_b
        mean_b = (nb * mean_b + nc * mc) / nn
        s_b = s_b + m2 + d * d * nb * nc / nn
        nb = nn
    n2, n = float(N), n1 + float(N)
    delta = M - mean_b
    return n, (n1 * M + n2 * mean_b) / n, S + s_b + delta * delta * n1 * n2 / n
