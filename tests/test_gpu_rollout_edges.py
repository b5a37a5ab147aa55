"""The rollout plane past its first workgroup, chunk and block (needs an MI355X).

The env-side filter (k_filter_chunk / k_filter_merge), the per-policy filter (k_zstats), observe,
reward, GAE with its standardization sums and ddrl_adv_sums_get, at the env counts where each
kernel leaves its first unit of work ("Rollout plane boundaries"):

  1. rollout + GAE parity (the assertions and tolerances of tests/test_gpu_parity.py) at env counts
     of several filter chunks, reward blocks and GAE wave groups;
  2. the env-side filter driven directly: fresh, frozen, disabled, other clips, and hard columns
     against a long-double two-pass reference, bounded by the fp64 oracle's own deviation;
  3. GAE driven directly over every branch of the chunked loop, with scripted done flags, and the
     standardization totals against math.fsum of the advantages the kernel wrote.
"""
import math

import numpy as np
import pytest

from ddrl_amd import native as N
from oracle import ddrl_oracle as O
from tests import rollout_edge_inputs as E
from tests.gpu_harness import OracleRollout, dev, filter_state, init_params, make_ctx, run_rollout, synthetic_inputs

pytestmark = pytest.mark.gpu
CENTRAL, SHARED, LOCAL, GLOBALCOST = E.CENTRAL, E.SHARED, E.LOCAL, E.GLOBALCOST
PFILTER = {"observation_filter": "MeanStdFilter"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddrl_amd import build
    build.build()


def _close(a, b, rtol=1e-5, atol=1e-5, msg=""):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=msg)


def _check_adv_sums(ctx, p, T, msg=""):
    """ddrl_adv_sums_get (s1, s2, n) of the last gae(): n = C T exactly; s1, s2 against math.fsum
    over the fp32 advantages the kernel wrote (exact fp64 terms: a product of two fp32 values has
    48 significant bits), so the reduction is isolated from the recursion.  Any summation order of
    n fp64 terms is within (n - 1) u sum|term| (1 + O(n u)) of the exact sum, u = 2^-53; the bound
    is n u sum|term|.  adv_norm follows from the totals."""
    lay = ctx.layout[p]
    s1, s2, n = ctx.adv_sums_get(p)
    assert n == lay["C"] * T, (msg, n, lay["C"], T)
    adv = ctx.records_get(p)[:, lay["adv"]].astype(np.float64)
    assert adv.size == n
    r1, r2 = math.fsum(adv), math.fsum(adv * adv)
    b1, b2 = n * 2.0 ** -53 * math.fsum(np.abs(adv)), n * 2.0 ** -53 * r2
    assert abs(s1 - r1) <= b1, (msg, "sum adv", s1, r1, b1)
    assert abs(s2 - r2) <= b2, (msg, "sum adv^2", s2, r2, b2)
    mean = s1 / n
    std = math.sqrt(max(s2 / n - mean * mean, 0.0))
    want = np.array([mean, max(np.float32(1e-4), np.float32(std))], np.float32)
    _close(ctx.adv_norm_get(p), want, rtol=1e-5, atol=1e-6, msg=f"{msg} adv_norm from the totals")
    return s1, s2, n


# ---- 1. rollout + GAE parity at multi-unit env counts ---------------------------------------
ROLLOUT_EDGES = [pytest.param(env, n, T, config, id=name) for name, env, n, T, config in E.ROLLOUT_EDGES]


@pytest.mark.parametrize("env,n,T,config", ROLLOUT_EDGES)
def test_rollout_gae_parity_multi_unit(env, n, T, config):
    """The assertions of tests/test_gpu_parity.py::_rollout_gae_parity, at the same tolerances,
    plus the standardization totals.  The heads are scaled by E.HEAD_SCALE, at which fp32 rounding
    of the sampled action cannot carry logp past its tolerance (guarded on the CPU)."""
    ctx, cfg, inst = make_ctx(env, n, T, config)
    want_mode = {GLOBALCOST: N.REWARD_GLOBAL}.get(env, N.REWARD_NORM if config else N.REWARD_PER_LEG)
    assert cfg.reward_mode == want_mode
    rng = np.random.default_rng(E.ROLLOUT_SEED)
    params = init_params(ctx, cfg, E.PARAM_SEED, head_scale=E.HEAD_SCALE)
    orc, norms, a_gpu, a_orc = run_rollout(ctx, cfg, inst, params, rng, E.rollout_filter_prior(cfg.obs_full_dim, rng), T)
    _close(a_gpu, a_orc, msg="env actions")
    assert 0.1 < (np.abs(a_orc) == 1).mean() < 0.6     # clipped and unclipped actions
    fn, fM, fS = ctx.filter_get()
    assert fn == orc.rs.n == 1000 + (T + 1) * n
    _close(fM, orc.rs.M, rtol=1e-12, atol=1e-12)
    _close(fS, orc.rs.S, rtol=1e-10, atol=1e-9)
    for p in range(cfg.n_policies):
        lay = ctx.layout[p]
        got = ctx.records_get(p)
        ref = orc.flat_records(p, lay)
        d, A = cfg.obs_dim[p], cfg.act_dim
        for name, sl in [("obs", slice(lay["obs"], lay["obs"] + d)),
                         ("act", slice(lay["act"], lay["act"] + A)),
                         ("logits", slice(lay["logit"], lay["logit"] + 2 * A)),
                         ("logp", lay["logp"]), ("vf", lay["vf"]), ("rew", lay["rew"]),
                         ("adv", lay["adv"]), ("vt", lay["vt"])]:
            _close(got[:, sl], ref[:, sl], rtol=1e-5, atol=2e-5, msg=f"{env} p{p} {name}")
        _close(ctx.last_values_get(p), orc.last_v[p], msg="bootstrap V(s_T)")
        an = ctx.adv_norm_get(p)
        _close(an, np.array(norms[p], np.float32), rtol=1e-5, atol=1e-6, msg="adv mean/std")
        _check_adv_sums(ctx, p, T, msg=f"{env} p{p}")
    assert orc.done.any()
    ctx.close()


@pytest.mark.parametrize("env,n", [pytest.param(LOCAL, 300, id="local300"), pytest.param(SHARED, 257, id="shared257")])
def test_policy_mean_std_filter_multi_unit(env, n):
    """k_zstats' stride loop with some threads taking two rows (n > 256): the assertions of
    tests/test_gpu_parity.py::test_rollout_with_policy_mean_std_filter."""
    T = 3
    ctx, cfg, inst = make_ctx(env, n, T, PFILTER)
    assert cfg.policy_filter == 1
    rng = np.random.default_rng(17)
    params = init_params(ctx, cfg, 4)
    orc, norms, a_gpu, a_orc = run_rollout(ctx, cfg, inst, params, rng, filter_state(cfg.obs_full_dim, rng), T)
    _close(a_gpu, a_orc, msg="env actions")
    for p in range(cfg.n_policies):
        pn, pM, pS = ctx.policy_filter_get(p)
        assert pn == orc.pf[p].n == (T + 1) * ctx.layout[p]["C"]
        _close(pM, orc.pf[p].M, rtol=1e-10, atol=1e-10)
        _close(pS, orc.pf[p].S, rtol=1e-9, atol=1e-8)
        dn, dM, dS = ctx.policy_filter_get(p, delta=True)
        assert dn == pn   # no sync yet: the delta is everything pushed
        lay = ctx.layout[p]
        got, ref = ctx.records_get(p), orc.flat_records(p, lay)
        d, A = cfg.obs_dim[p], cfg.act_dim
        _close(got[:, :d], ref[:, :d], rtol=1e-5, atol=2e-5, msg="filtered obs")
        _close(got[:, lay["logit"]:lay["logit"] + 2 * A], ref[:, lay["logit"]:lay["logit"] + 2 * A],
               rtol=1e-5, atol=2e-5, msg="logits")
    pn, pM, pS = ctx.policy_filter_get(0)
    ctx.policy_filter_set(0, pn, pM * 0.5, pS)
    n2, M2, _ = ctx.policy_filter_get(0)
    assert n2 == pn and np.array_equal(M2, pM * 0.5)
    ctx.close()


# ---- 2. the env-side filter, driven directly ---------------------------------------------------
# Centralized: one policy whose 43 inputs are the 43 observation columns, one row per env, so the
# record's observation field at T = 1 is the normalized observation, routed by obs_indices.
def _filter_ctx(n, config=None, cfg_set=None, seed=2):
    ctx, cfg, inst = make_ctx(CENTRAL, n, 1, config, cfg_set=cfg_set)
    assert cfg.n_policies == 1 and cfg.obs_dim[0] == cfg.obs_full_dim == 43
    params = init_params(ctx, cfg, seed)
    route = list(inst.obs_indices["central_agent"])
    assert sorted(route) == list(range(43))
    return ctx, cfg, inst, params, route


def _observed_rows(ctx, cfg, obs):
    """observe, then act at t = 0: the normalized, routed rows as the record holds them."""
    import torch
    n = cfg.n_envs
    ctx.observe(dev(obs))
    eps = torch.zeros((n, cfg.n_agents, cfg.act_dim), dtype=torch.float32, device="cuda")
    actions = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    ctx.act(0, eps, actions)
    ctx.synchronize()
    lay = ctx.layout[0]
    return ctx.records_get(0)[:, lay["obs"]:lay["obs"] + cfg.obs_dim[0]]


def _check_filter_state(got, rs_n, rs_M, rs_S, msg):
    n, M, S = got
    assert n == rs_n, (msg, n, rs_n)
    _close(M, rs_M, rtol=1e-12, atol=1e-12, msg=f"{msg} M")
    _close(S, rs_S, rtol=1e-10, atol=1e-9, msg=f"{msg} S")


@pytest.mark.parametrize("n", [1, 2, 256, 257])
def test_fresh_filter_updating(n):
    """n = 0, M = S = 0, two pushes of n rows: count, M, S and the delta buffer against the oracle's
    per-row pushes; the normalized rows of both pushes.  After the first push of one row the
    reference's quirk holds: n = 1 gives var = M^2, so z = (x - x) / (|x| + 1e-8) = 0 exactly."""
    ctx, cfg, inst, params, route = _filter_ctx(n)
    D = cfg.obs_full_dim
    ctx.filter_set(0.0, np.zeros(D), np.zeros(D))
    ctx.filter_delta_reset()
    obs = synthetic_inputs(np.random.default_rng(23 + n), cfg, 1)[0]
    obs[0, :, 5] = 0.0    # a zero column: M = 0, std = 0 + 1e-8 after one row
    orc = OracleRollout(cfg, inst, params, (0, np.zeros(D), np.zeros(D)))
    for push in range(2):
        rows = _observed_rows(ctx, cfg, obs[push])
        orc.observe(obs[push])
        assert orc.rs.n == (push + 1) * n
        _check_filter_state(ctx.filter_get(), orc.rs.n, orc.rs.M, orc.rs.S, f"push {push}")
        _check_filter_state(ctx.filter_delta_get(), orc.rs.n, orc.rs.M, orc.rs.S, f"push {push} delta")
        _close(rows, orc.stage[0], rtol=1e-5, atol=2e-5, msg=f"push {push} normalized rows")
        if n == 1 and push == 0:
            assert np.all(obs[0][:, [c for c in range(D) if c != 5]] != 0)
            assert np.array_equal(rows, np.zeros_like(rows))
        elif n > 1:
            assert np.abs(rows).max() > 0.5
    ctx.close()


def test_fresh_filter_frozen():
    """n = 0 and filter_update = 0: the constants are (0, sqrt(0 * 0) + 1e-8), so z = clip(x / 1e-8):
    every nonzero input lands on +-clip and zero stays zero, exactly, and nothing is pushed."""
    n = 257
    ctx, cfg, inst, params, route = _filter_ctx(n, cfg_set={"filter_update": 0})
    D = cfg.obs_full_dim
    ctx.filter_set(0.0, np.zeros(D), np.zeros(D))
    ctx.filter_delta_reset()
    obs = synthetic_inputs(np.random.default_rng(29), cfg, 1)[0][0]
    obs[::3, 4] = 0.0
    obs[256, 9] = 0.0
    nz = obs[obs != 0]
    assert np.abs(nz).min() > 1e-6 and (obs == 0).sum() >= 87      # x / 1e-8 saturates every nonzero input
    rows = _observed_rows(ctx, cfg, obs)
    want = (np.sign(obs) * np.float32(cfg.filter_clip))[:, route]
    assert cfg.filter_clip == 10.0 and (want > 0).any() and (want < 0).any()
    np.testing.assert_array_equal(rows, want)
    for got in (ctx.filter_get(), ctx.filter_delta_get()):
        assert got[0] == 0 and not got[1].any() and not got[2].any()
    ctx.close()


def test_env_filter_disabled():
    """observation_filter_env False: the routed observations are the raw fp32 inputs bit for bit,
    and neither the filter state nor its count moves."""
    n = 257
    ctx, cfg, inst, params, route = _filter_ctx(n, {"env_config": {"observation_filter_env": False}})
    assert cfg.filter_enabled == 0
    rng = np.random.default_rng(31)
    filt = filter_state(cfg.obs_full_dim, rng)
    ctx.filter_set(*filt)
    ctx.filter_delta_reset()
    obs = synthetic_inputs(rng, cfg, 1)[0][0]
    obs[:, 3] *= 1e4    # far beyond any clip
    rows = _observed_rows(ctx, cfg, obs)
    np.testing.assert_array_equal(rows, obs[:, route])
    fn, fM, fS = ctx.filter_get()
    assert fn == filt[0] and np.array_equal(fM, filt[1]) and np.array_equal(fS, filt[2])
    dn, dM, dS = ctx.filter_delta_get()
    assert dn == 0 and not dM.any() and not dS.any()
    ctx.close()


@pytest.mark.parametrize("clip", [2.5, 0.0])
def test_filter_clip_values(clip):
    """filter_clip 2.5: saturated entries are +-2.5 exactly, the rest match the oracle.  filter_clip
    0: nothing is clipped (the oracle treats a falsy clip the same way)."""
    n = 257
    ctx, cfg, inst, params, route = _filter_ctx(n, {"env_config": {"filter_clip": clip}})
    assert cfg.filter_clip == clip
    rng = np.random.default_rng(37)
    filt = filter_state(cfg.obs_full_dim, rng)
    ctx.filter_set(*filt)
    obs = synthetic_inputs(rng, cfg, 1)[0][0]
    for j in range(0, 43, 4):    # two outliers per column: z = sqrt(1257 / 2) = 25 whatever the spread
        obs[[j, 256 - j], j] = (300.0, -300.0)
    orc = OracleRollout(cfg, inst, params, filt)
    rows = _observed_rows(ctx, cfg, obs)
    orc.observe(obs)
    ref = orc.stage[0]
    _check_filter_state(ctx.filter_get(), orc.rs.n, orc.rs.M, orc.rs.S, f"clip {clip}")
    _close(rows, ref, rtol=1e-5, atol=2e-5, msg=f"clip {clip}")
    if clip:
        hi, lo = ref == np.float32(clip), ref == -np.float32(clip)
        assert hi.sum() > 100 and lo.sum() > 100 and (np.abs(ref) < clip).sum() > ref.size // 2
        assert np.abs(ref).max() == clip and np.abs(rows).max() == clip
        np.testing.assert_array_equal(rows[hi | lo], ref[hi | lo])
    else:
        assert (ref > 10.0).sum() >= 11 and (ref < -10.0).sum() >= 11
        assert np.array_equal(np.abs(rows) > 10.0, np.abs(ref) > 10.0)
    ctx.close()


@pytest.mark.parametrize("kind", ["fresh", "prior", "matched"])
def test_filter_hard_columns(kind):
    """N = 513 (three chunks, the last of one row), 4 pushes; one column with mean 1000 and std 2e-3
    as fp32 inputs, one constant column.  Reference: the two-pass mean and M2 of all pushed rows
    in long double, merged with the prior by Chan's formula in long double -- not the per-row
    oracle, whose own error is what bounds the test: per column the kernel's relative deviation
    from the reference in M and in S is at most 4 x the fp64 oracle's deviation from the same
    reference (the factor allows for a different summation order), floored at 64 ulp (1.4e-14).
    S of the constant column is exactly the prior's S, or 0 when fresh.  Prints the measured pairs
    (-s)."""
    assert np.finfo(np.longdouble).eps < 1e-18   # the reference needs an extended long double
    n, pushes = 513, 4
    ctx, cfg, inst, params, route = _filter_ctx(n)
    D = cfg.obs_full_dim
    prior = E.hard_filter_prior(D, kind)
    obs = E.hard_filter_pushes(n, D, pushes)
    ctx.filter_set(*prior)
    rs = O.RunningStat((D,))
    rs.n, rs.M[:], rs.S[:] = int(prior[0]), prior[1], prior[2]
    for k in range(pushes):
        ctx.observe(dev(obs[k]))
        for row in obs[k]:
            rs.push(row)
    ctx.synchronize()
    gn, gM, gS = ctx.filter_get()
    rn, rM, rS = E.longdouble_filter_reference(prior, obs)
    assert gn == rs.n == float(rn) == prior[0] + pushes * n
    floor = 64 * 2.0 ** -52
    for name, got, orc, ref in (("M", gM, rs.M, rM), ("S", gS, rs.S, rS)):
        dk, do = E.relative_deviation(got, ref), E.relative_deviation(orc, ref)
        bound = np.maximum(4 * do, floor)
        worst = int(np.argmax(dk / bound))
        print(f"\nfilter {kind} {name}: max relative deviation from long double: kernel {float(dk.max()):.3g} "
              f"(column {int(np.argmax(dk))}), fp64 oracle {float(do.max()):.3g} (column {int(np.argmax(do))}); "
              f"hard column kernel {float(dk[E.HARD_COL]):.3g} / oracle {float(do[E.HARD_COL]):.3g}; "
              f"worst kernel / bound {float(dk[worst] / bound[worst]):.3g} (column {worst})")
        assert np.all(dk <= bound), (kind, name, np.flatnonzero(dk > bound), dk[dk > bound], bound[dk > bound])
    assert gS[E.CONST_COL] == prior[2][E.CONST_COL] and gM[E.CONST_COL] == float(E.CONST_VAL)
    ctx.close()


# ---- 3. GAE and standardization, driven directly -----------------------------------------------
def _run_gae(T, n, k, rew, vf, done, last_v, config=None):
    ctx, cfg, _ = make_ctx(CENTRAL if k == 1 else SHARED, n, T, config)
    lay = ctx.layout[0]
    C = n * k
    assert cfg.n_policies == 1 and lay["C"] == C
    rec = np.zeros((T * C, lay["stride"]), np.float32)
    rec[:, lay["rew"]] = rew.reshape(-1)
    rec[:, lay["vf"]] = vf.reshape(-1)
    ctx.records_set(0, rec)
    ctx.done_set(done)
    ctx.last_values_set(0, last_v)
    ctx.gae()
    ctx.synchronize()
    got = ctx.records_get(0)
    return ctx, cfg, got[:, lay["adv"]].reshape(T, C), got[:, lay["vt"]].reshape(T, C)


def _gae_case(T, n, k, config=None):
    rew, vf, done, last_v = E.gae_inputs(T, n, k)
    ctx, cfg, adv, vt = _run_gae(T, n, k, rew, vf, done, last_v, config)
    ref_adv, ref_vt = O.gae_fragment(rew, vf, np.repeat(done, k, axis=1), last_v, cfg.gamma, cfg.lambda_)
    _close(adv, ref_adv, rtol=1e-5, atol=2e-5, msg="advantages")
    _close(vt, ref_vt, rtol=1e-5, atol=2e-5, msg="value targets")
    _, mean, std = O.standardize(ref_adv.reshape(-1))
    _close(ctx.adv_norm_get(0), np.array([mean, max(np.float32(1e-4), std)], np.float32), rtol=1e-5, atol=1e-6,
           msg="adv mean/std")
    _check_adv_sums(ctx, 0, T, msg=f"T {T} n {n} k {k}")
    return ctx, cfg


@pytest.mark.parametrize("k", [1, 4], ids=["k1", "k4"])
@pytest.mark.parametrize("T,n", E.GAE_SHAPES)
def test_gae_direct(T, n, k):
    """Records, done flags and V(s_T) set directly; reference O.gae_fragment + O.standardize.
    k = 4: one done flag per env shared by its 4 chains (e = c / k)."""
    ctx, cfg = _gae_case(T, n, k)
    assert (cfg.gamma, cfg.lambda_) == (np.float32(0.99), np.float32(0.95))
    ctx.close()


@pytest.mark.parametrize("T,n,k", [(33, 70, 4), (17, 257, 1)])
def test_gae_direct_other_discounts(T, n, k):
    """gamma 0.9 / lambda 0.8 on the cfg before the context is made."""
    ctx, cfg = _gae_case(T, n, k, {"gamma": 0.9, "lambda": 0.8})
    assert (cfg.gamma, cfg.lambda_) == (np.float32(0.9), np.float32(0.8))
    ctx.close()


@pytest.mark.parametrize("k", [1, 4], ids=["k1", "k4"])
def test_gae_degenerate_statistics(k):
    """All-zero inputs give adv_norm = (0, 1e-4f) exactly.  T = 1, all done, vf = 0, rew = 0.1
    gives constant advantages, whose one-pass variance s2 / n - mean^2 may round negative: the
    result is std = 1e-4f with mean 0.1f."""
    n = 300
    for T in (3, 1):
        C = n * k
        if T == 3:
            rew, done = np.zeros((T, C), np.float32), np.zeros((T, n), np.uint8)
        else:
            rew, done = np.full((T, C), 0.1, np.float32), np.ones((T, n), np.uint8)
        ctx, cfg, adv, vt = _run_gae(T, n, k, rew, np.zeros((T, C), np.float32), done, np.zeros(C, np.float32))
        want = np.float32(0.0 if T == 3 else 0.1)
        assert np.array_equal(adv, np.full((T, C), want)) and np.array_equal(vt, adv)
        an = ctx.adv_norm_get(0)
        assert an[0] == want and an[1] == np.float32(1e-4), (T, an)
        s1, s2, cnt = _check_adv_sums(ctx, 0, T)
        assert cnt == C * T and (T == 1 or (s1 == 0 and s2 == 0))
        ctx.close()
