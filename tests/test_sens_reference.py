"""CPU checks of the sensitivity reference (tests/sens_reference.py) and of the host-side helpers:
the reference matrix converges to 2 h * d mean / d x, the default steps are the reference's
0.1 * rs.std, the seeded inputs of the device tests meet the bars those tests assert, and the new
entry points fail with a message without a context.

Reference: evaluation/rollout_episodes_compute_gradient.py:59-68, :111-122."""
import types

import numpy as np
import pytest

from ddrl_amd import build, evaluation, native as N
from ddrl_amd.spec import make_cfg
from oracle import ddrl_oracle as O
from tests import sens_reference as S
from tests.gpu_harness import OracleRollout, init_cup_params, make_params


def _jacobian(mod, params, x, A):
    """d mean_j / d x_f [d, A] of one row from the oracle's backward: for a single row the bias
    gradient of layer 1 is dz1, and dx = dz1 W1^T."""
    x = np.asarray(x)[None]
    cols = []
    for j in range(A):
        logits, _, cache = mod.ffn_forward(params, x)
        dl = np.zeros_like(logits)
        dl[0, j] = 1
        g = mod.ffn_backward(params, cache, dl, np.zeros(1))
        cols.append(g["fc_1/bias"] @ params["fc_1/kernel"].T)
    return np.stack(cols, 1)


def test_reference_matrix_converges_to_the_jacobian():
    O64 = O.with_dtype(np.float64)
    rng = np.random.default_rng(4)
    d, A = 5, 2
    params = {k: v.astype(np.float64) for k, v in O.ffn_init(rng, d, 2 * A).items()}
    x = rng.normal(size=d)
    mean = lambda v: O64.ffn_forward(params, v[None])[0][0, :A]
    assert (np.abs(mean(x)) < 1).all()
    J = _jacobian(O64, params, x, A)
    assert np.abs(J).max() > 1e-2
    errs = []
    for h in (1e-1, 1e-2, 1e-3):
        hs = np.full(d, h)
        errs.append(np.abs(S.fd_matrix(mean, x, hs) / (2 * hs[:, None]) - J).max())
    assert errs[1] < errs[0] / 50 and errs[2] < errs[1] / 50 and errs[2] < 1e-6, errs   # O(h^2)


def test_sens_means_is_the_central_difference_of_the_policy():
    """The whole reference path (routing, perturbation, fp32 forward, clip) on a small env with both
    filters off: x = z, so the fp32 differences are 2 h J up to O(h^3) and fp32 rounding."""
    cfg, inst = make_cfg("QuantrupedMultiEnv_SharedDecentral", 2, 3, {"env_config": {"observation_filter_env": False}})
    params = make_params(cfg, 5, head_scale=1.0)
    orc = OracleRollout(cfg, inst, params, (0.0, np.zeros(cfg.obs_full_dim), np.zeros(cfg.obs_full_dim)))
    rng = np.random.default_rng(2)
    obs = rng.normal(size=(2, cfg.obs_full_dim)).astype(np.float32)
    d, A, h = cfg.obs_dim[0], cfg.act_dim, 0.05
    (x, base, moved), = S.perturbed_inputs(orc, obs, [np.full(d, h)])
    assert x.shape == (2 * d, 8, d) and moved.all()
    for f in range(d):   # only feature f differs from the base row, by -h / +h
        for r, sign in ((2 * f, -1), (2 * f + 1, 1)):
            delta = x[r].astype(np.float64) - base
            np.testing.assert_allclose(delta[:, f], sign * h, atol=1e-6)
            assert (np.delete(delta, f, 1) == 0).all()
    (means, base_means, _), = S.sens_means(orc, obs, [np.full(d, h)])
    assert (np.abs(base_means) < 1).all()
    terms = S.terms(means)
    p64 = {k: v.astype(np.float64) for k, v in params[0].items()}
    O64 = O.with_dtype(np.float64)
    for c in range(8):
        J = _jacobian(O64, p64, base[c].astype(np.float64), A)
        np.testing.assert_allclose(terms[c], 2 * h * J, atol=2e-4 * np.abs(J).max() + 1e-6)
    acc = S.SensAccumulator(cfg)
    acc.step([means], np.array([True, False]))
    assert acc.rows == [4]
    np.testing.assert_allclose(acc.grads[0], terms[:4].astype(np.float64).sum(0), rtol=1e-12)
    np.testing.assert_array_equal(acc.grads_abs[0], acc.mag[0])


def test_default_steps_are_a_tenth_of_the_filter_std():
    rs = O.RunningStat((7,))
    for row in np.random.default_rng(1).normal(size=(50, 7)) * np.arange(1, 8):
        rs.push(row)
    np.testing.assert_allclose(evaluation.default_sens_steps(rs.n, rs.S, 0.1, rs.M), 0.1 * rs.std, rtol=1e-15)
    np.testing.assert_allclose(evaluation.default_sens_steps(rs.n, rs.S), 0.1 * np.sqrt(rs.S / 49), rtol=1e-15)
    np.testing.assert_array_equal(S.default_steps(rs.n, rs.S, rs.M), 0.1 * rs.std)
    one = O.RunningStat((3,))
    one.push(np.array([1.0, -2.0, 0.0]))   # n = 1: RLlib's RunningStat reports var = M^2
    np.testing.assert_array_equal(evaluation.default_sens_steps(one.n, one.S, 0.5, one.M), 0.5 * one.std)
    assert (evaluation.default_sens_steps(0, np.zeros(3)) == 0).all()


@pytest.mark.parametrize("name", list(S.ORACLE_CASES))
def test_seeded_inputs_meet_the_bars_of_the_device_test(name):
    """test_matrices_match_the_oracle asserts that at least half of the base means are unclipped and
    that at least 90 % of the non-constant entries of grads_abs are non-zero: the seeded inputs
    have to make that true of the oracle."""
    cfg, inst, config, filt, pfilt, obs, steps = S.oracle_case(name)
    if name == "central_tvel3":
        assert cfg.obs_dim[0] == 44 and cfg.act_dim == 8 and cfg.obs_full_dim == 44
    if S.is_cup(config):
        params = init_cup_params(types.SimpleNamespace(params_set=lambda *a: None), cfg, 5, head_scale=1.0)
    else:
        params = make_params(cfg, 5, head_scale=1.0)
    orc = S.make_oracle(cfg, inst, config, params, filt, pfilt)
    acc = S.SensAccumulator(cfg)
    inside = total = 0
    for t in range(S.T):
        res = S.sens_means(orc, obs[t], steps)
        acc.step([r[0] for r in res])
        inside += sum(int((np.abs(r[1]) < 1).sum()) for r in res)
        total += sum(r[1].size for r in res)
    assert inside * 2 >= total, (inside, total)
    for p in range(cfg.n_policies):
        const = ~res[p][2].any(0)
        assert const.sum() == (4 if name == "legid3" else 0)
        assert (acc.grads_abs[p][const] == 0).all()
        assert (acc.grads_abs[p][~const] != 0).mean() >= 0.9
        assert acc.rows[p] == S.T * cfg.n_envs * res[p][2].shape[0]


def test_entry_points_fail_with_messages_without_a_context():
    build.build()
    lib = N.load()
    for rc in (lib.ddrl_eval_sens_begin(None, None), lib.ddrl_eval_sens(None, None, None),
               lib.ddrl_eval_sens_results(None, 0, None, None, None)):
        assert rc == -1 and b"null context" in lib.ddrl_last_error()
