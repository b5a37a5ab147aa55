"""CPU guards of the rollout-plane boundary tests' inputs and references (no GPU): the scripted
done patterns hold every class the GPU tests rely on, and the long-double filter reference bounds
the kernel's chunk order (emulated in numpy fp64) by the fp64 oracle's own deviation."""
import numpy as np
import pytest

from oracle import ddrl_oracle as O
from tests import eval_reference as R
from tests import rollout_edge_inputs as E


@pytest.mark.parametrize("T,n", E.GAE_SHAPES)
def test_gae_done_pattern_covers_every_class(T, n):
    """Each shape holds every class it has room for: a done at t = T - 1, at t = 0, on either side
    of the chunk seam (t = T - 16 and T - 17), a chain done at every step, one never done; from 8
    envs on also columns with several random flags."""
    done = E.gae_done_pattern(T, n)
    assert done.shape == (T, n) and done.dtype == np.uint8
    c = E.gae_done_classes(done)
    if T == 1:      # one step: a done at T - 1 is a done at 0 is a done at every step
        assert c["always"] >= 1 and (n < 6 or c["never"] >= 1), c
        return
    assert c["last_only"] >= 1 and c["first_only"] >= 1 and c["always"] >= 1, c
    assert c["seam_hi_only"] >= (T >= 16) and c["seam_lo_only"] >= (T >= 17), c
    assert n < 6 or c["never"] >= 1, c
    assert n < 64 or c["mixed"] >= 1, c


def test_gae_shapes_cover_every_loop_branch():
    """The shapes hit 1, 2, 3 and 4 chunks, each with a full and a ragged last chunk, one wave and
    several, ragged waves, and one group and several with full and ragged last groups."""
    chunks = {((T + 15) // 16, T % 16 == 0) for T, _ in E.GAE_SHAPES}
    assert chunks == {(1, False), (1, True), (2, False), (2, True), (3, False), (3, True), (4, False)}
    waves = {(C + 63) // 64 for _, n in E.GAE_SHAPES for C in (n, 4 * n)}
    groups = {(C + 255) // 256 for _, n in E.GAE_SHAPES for C in (n, 4 * n)}
    assert {1, 2, 3, 5, 9} <= waves and {1, 2, 3, 5} <= groups
    assert any(n % 64 == 0 for _, n in E.GAE_SHAPES) and any(((4 * n + 63) // 64) % 4 == 0 for _, n in E.GAE_SHAPES)


@pytest.mark.parametrize("n", [64, 70])
def test_eval_done_pattern_covers_every_class(n):
    """The 12 x n pattern of the multi-block accounting cases, in the envs of the last block too
    (n = 70: envs 64..69 hold an end within the quota, and the pattern as a whole every class)."""
    done = R.scripted_done(12, n)
    c = R.done_classes(done, 2)
    assert all(v >= 3 for k, v in c.items() if k != "no_episode") and c["no_episode"] >= 1, c
    if n > 64:
        assert done[:, 64:].any() and not done[:, 64:].all(), "the second block records episodes"


def test_scripted_done_is_the_seeded_pattern():
    """R.scripted_done is the expression the accounting tests have always used."""
    want = (np.random.default_rng(41).random((12, 37)) < 0.25).astype(np.uint8)
    assert np.array_equal(R.scripted_done(12, 37), want)
    c = R.done_classes(want, 2)
    assert all(v >= 3 for k, v in c.items() if k != "no_episode") and c["no_episode"] >= 1, c


@pytest.mark.parametrize("kind", ["fresh", "prior", "matched"])
@pytest.mark.parametrize("n", [1, 257, 513])
def test_filter_reference_bounds_the_chunk_order(n, kind):
    """The bound of test_filter_hard_columns holds for the kernel's chunk order emulated in numpy
    fp64: per column its relative deviation from the long-double reference is at most 4 x the
    per-row fp64 oracle's, floored at 64 ulp; the constant column's S does not move."""
    assert np.finfo(np.longdouble).eps < 1e-18
    D = 43
    prior = E.hard_filter_prior(D, kind)
    obs = E.hard_filter_pushes(n, D, 4)
    assert obs.dtype == np.float32 and np.all(obs[:, :, E.CONST_COL] == E.CONST_VAL)
    hard = obs[:, :, E.HARD_COL].astype(np.float64)
    assert abs(hard.mean() - 1000) < 5e-3 and (n == 1 or 1e-3 < hard.std() < 4e-3)
    rs = O.RunningStat((D,))
    rs.n, rs.M[:], rs.S[:] = int(prior[0]), prior[1], prior[2]
    state = prior
    for k in range(4):
        state = E.emulate_chunked_push(state, obs[k])
        for row in obs[k]:
            rs.push(row)
    rn, rM, rS = E.longdouble_filter_reference(prior, obs)
    assert state[0] == rs.n == float(rn)
    floor = 64 * 2.0 ** -52
    for got, orc, ref in ((state[1], rs.M, rM), (state[2], rs.S, rS)):
        dk, do = E.relative_deviation(got, ref), E.relative_deviation(orc, ref)
        assert np.all(dk <= np.maximum(4 * do, floor)), (dk.max(), do.max())
    assert state[2][E.CONST_COL] == prior[2][E.CONST_COL] == rs.S[E.CONST_COL]
    # the per-row oracle stays within the parity tests' bounds of the reference (M 1e-12, S 1e-10)
    np.testing.assert_allclose(rs.M, np.asarray(rM, np.float64), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(rs.S, np.asarray(rS, np.float64), rtol=1e-10, atol=1e-9)


def _logp_bound_over_tolerance(env, n, T, config, head_scale):
    from ddrl_amd.spec import make_cfg
    from tests.gpu_harness import make_params, oracle_rollout
    cfg, inst = make_cfg(env, n, T, config)
    rng = np.random.default_rng(E.ROLLOUT_SEED)
    params = make_params(cfg, E.PARAM_SEED, head_scale)
    orc, _ = oracle_rollout(cfg, inst, params, rng, E.rollout_filter_prior(cfg.obs_full_dim, rng), T)
    ratios = []
    for r in orc.rec:
        tol = E.LOGP_RTOL * np.abs(r["logp"]) + E.LOGP_ATOL
        ratios.append((E.logp_rounding_bound(r["logits"], r["act"]) / tol).reshape(-1))
    return np.concatenate(ratios)


@pytest.mark.parametrize("name,env,n,T,config", E.ROLLOUT_EDGES, ids=[c[0] for c in E.ROLLOUT_EDGES])
def test_rollout_edge_logp_is_well_conditioned(name, env, n, T, config):
    """From the oracle alone: at E.HEAD_SCALE the rounding of the sampled action moves no row's
    fp32 logp by more than a quarter of the parity tolerance, so the tolerance is a statement about
    the kernel and not about which way a = fl(mu + std eps) rounds."""
    ratio = _logp_bound_over_tolerance(env, n, T, config, E.HEAD_SCALE)
    assert ratio.max() <= 0.25, ratio.max()


def test_logp_tolerance_is_not_implied_at_head_scale_30():
    """The same measure with the heads scaled 30 x, as the small-batch parity tests have them: at
    257 envs x T = 3 several rows can move past the tolerance by rounding alone, which is why the
    multi-unit cases do not use that scale."""
    _, env, n, T, config = E.ROLLOUT_EDGES[0]
    ratio = _logp_bound_over_tolerance(env, n, T, config, 30.0)
    assert ratio.max() > 2 and 5 <= (ratio > 1).sum() < 0.02 * ratio.size, (ratio.max(), (ratio > 1).sum())
