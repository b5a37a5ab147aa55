"""The fused row-split update's forward against the plain forward in the same library, and
against the oracle (needs an MI355X).

ppo_ffn.hip's kernels run ffn_fwd_rt with its head's Wo rows read ahead of the tail (HEADPF:
issue order only; every output is still the sum over (fb, r) ascending, then qsum, then + bo)
in every value branch and in the A = 2 policy branches other than the cup model's; the A = 4
and A = 8 policy branches and the cup policy branch keep the plain tail.  ppo_ffn_atomic.hip
builds the same update with the plain forward everywhere and sums the same LSB-replaced
partials, so a context made under DDRL_XCHG=atomic is the old forward in the same library: the
two must leave the same bits in the parameters, Adam's moments and the statistics.  (On the
parent commit, where both translation units ran the same forward, the two protocols were
bit-equal at every shape below.)

One registry env per (A, KS1, cup) instance of the fused row-split dispatch that the registry
reaches -- (2, 5), (2, 7), (2, 9), (2, 12: d = 23 takes the zero-padded generic instance, whose
layer-1 k-steps 6 - 11 meet only zero rows), (4, 7), (8, 11) and the cup model; in the last three
only the value branch's head differs between the two translation units.  No registered env has
A = 2 with d in 41 .. 44, or A = 4 / A = 8 outside KS1 = 7 / 11, so <2, 11>, <4, 12> and <8, 12>
have no case: the head's code does not depend on KS1, and their KS1 is run by (8, 11) and
(2, 12).  Every case: 8 envs, T such that R = 256 rows (two minibatches), 4 steps on the oracle's
batch, fed as test_gpu_update_tail._setup feeds it.

Bars: bit equality between the two forwards (assert_array_equal); the oracle parity at
test_gpu_parity's bars (_params_close, strict_params_check, statistics rtol 1e-4 / atol 1e-5).
"""
import numpy as np
import pytest

from oracle import ddrl_oracle as O
from tests import test_gpu_parity as TP
from tests.gpu_harness import (CUP_CONFIG, CUP_ENV, CupOracleRollout, filter_state, init_cup_params, init_params,
                               make_ctx, run_rollout, strict_params_check)

pytestmark = pytest.mark.gpu
STEPS = 4

CASES = [
    pytest.param(("QuantrupedMultiEnv_SharedDecentral", 8, None, 2, 19), id="A2-KS5"),
    pytest.param(("QuantrupedMultiEnv_SingleNeighbor", 32, None, 2, 27), id="A2-KS7"),
    pytest.param(("QuantrupedMultiEnv_Local", 32, None, 2, 35), id="A2-KS9"),
    pytest.param(("QuantrupedMultiEnv_SharedDecentralLegID", 8, None, 2, 23), id="A2-KS12"),
    pytest.param(("QuantrupedMultiEnv_TwoSides", 32, None, 4, 27), id="A4-KS7"),
    pytest.param(("QuantrupedMultiEnv_Centralized", 32, None, 8, 43), id="A8-KS11"),
    pytest.param((CUP_ENV, 8, CUP_CONFIG, 2, 19), id="cup-KS5"),
]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddrl_amd import build
    build.build()


def _is_cup(config):
    return config is CUP_CONFIG


def _state(ctx, cfg):
    """(parameters, m, v, beta powers, statistics) of every policy."""
    out = []
    for p in range(cfg.n_policies):
        m, v, b1p, b2p = ctx.adam_get(p)
        out.append((ctx.params_get(p), np.asarray(m), np.asarray(v), (b1p, b2p), ctx.ppo_stats(p, STEPS)))
    return out


@pytest.fixture(scope="module", params=CASES)
def case(request):
    """The update run once under each protocol on the oracle's batch, and what the oracle needs:
    shared, unchanged, by the tests below."""
    import torch
    env, T, config, A_want, d_want = request.param
    cup = _is_cup(config)
    init = (lambda c, g: init_cup_params(c, g, 7, head_scale=1.0)) if cup else (lambda c, g: init_params(c, g, 7, head_scale=1.0))
    ctx, cfg, inst = make_ctx(env, 8, T, config)
    rng = np.random.default_rng(5)
    params = init(ctx, cfg)
    orc, norms, _, _ = run_rollout(ctx, cfg, inst, params, rng, filter_state(cfg.obs_full_dim, rng), T,
                                   **({"orc_cls": CupOracleRollout} if cup else {}))
    P = cfg.n_policies
    recs = [orc.flat_records(p, ctx.layout[p]) for p in range(P)]
    shuffles, perms, kls = [], [], []
    for p in range(P):
        R = T * ctx.layout[p]["C"]
        assert R == 256 and cfg.obs_dim[p] == d_want and cfg.act_dim == A_want
        sh, pe = O.sgd_schedule(np.random.default_rng(100 + p), R, 128, cfg.num_sgd_iter)
        shuffles.append(sh)
        perms.append(pe)
        kls.append(0.2 + 0.1 * p)
    dsh = [torch.from_numpy(s).cuda() for s in shuffles]
    dpe = [torch.from_numpy(s).cuda() for s in perms]

    def run(c):
        for p in range(P):
            c.records_set(p, recs[p])
            c.adv_norm_set(p, *norms[p])
        c.ppo_update((1 << P) - 1, dsh, dpe, kls, max_steps=STEPS)
        c.synchronize()
        return _state(c, cfg)

    got = run(ctx)
    layout = [dict(ctx.layout[p]) for p in range(P)]
    ctx.close()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DDRL_XCHG", "atomic")   # read when the context is made: the atomic translation unit
        actx, acfg, _ = make_ctx(env, 8, T, config)
    init(actx, acfg)
    old = run(actx)
    actx.close()
    return dict(env=env, cfg=cfg, cup=cup, params=params, recs=recs, norms=norms, layout=layout,
                shuffles=shuffles, perms=perms, kls=kls, got=got, old=old)


def test_same_bits_as_old_forward(case):
    for p, (g, o) in enumerate(zip(case["got"], case["old"])):
        for name, a, b in zip(("params", "adam m", "adam v", "beta powers", "ppo_stats"), g, o):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=f"{case['env']} p{p} {name}")
        assert np.any(g[0] != O.pack(case["params"][p], _shapes(case, p))), "the update did not run"


def _shapes(case, p):
    d, A = case["cfg"].obs_dim[p], case["cfg"].act_dim
    return O.cup_param_shapes(d, A) if case["cup"] else O.ffn_param_shapes(d, 2 * A)


def test_oracle_parity(case):
    cfg, cup = case["cfg"], case["cup"]
    model = "cup" if cup else "ffn"
    for p in range(cfg.n_policies):
        lay, d, A = case["layout"][p], cfg.obs_dim[p], cfg.act_dim
        batch = TP._batch_from_records(case["recs"][p], lay, d, A, case["norms"][p])
        if cup:
            batch["leg"] = case["recs"][p][:, lay["leg"]].astype(np.int64)
        shapes = _shapes(case, p)
        adam = O.Adam(sum(int(np.prod(s)) for _, s in shapes), lr=cfg.lr)
        new, stats = O.ppo_update(model, case["params"][p], shapes, adam, batch, case["shuffles"][p], case["perms"][p],
                                  np.float32(case["kls"][p]), {"entropy_coeff": 0.0}, steps=STEPS)
        got, _, _, (b1p, b2p), st = case["got"][p]
        msg = f"{case['env']} p{p}"
        TP._params_close(got, O.pack(new, shapes), cfg.lr, STEPS, msg)
        strict_params_check(got, model, case["params"][p], shapes, batch, case["shuffles"][p], case["perms"][p],
                            case["kls"][p], STEPS, lr=cfg.lr, msg=msg)
        assert b1p == np.float32(adam.b1p) and b2p == np.float32(adam.b2p)
        for k, s in enumerate(stats):
            want = [s["total_loss"], s["policy_loss"], s["vf_loss"], s["kl"], s["entropy"],
                    s["vf_explained_var"], s["grad_gnorm"]]
            TP._close(st[k, :7], np.array(want, np.float32), rtol=1e-4, atol=1e-5, msg=f"{msg} stats step {k}")
