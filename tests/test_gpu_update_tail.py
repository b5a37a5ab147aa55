"""Fused update at observation widths whose last W1 feature block holds only a few rows
(needs an MI355X).

d = 35 / 36 (Local) and d = 19 / 20 (the decentral envs) leave 3 or 4 valid rows in the last
16-row block of W1; d = 27 (SingleNeighbor) is the control with 11.  Every case runs 4 steps
(2 epochs x 2 minibatches of a 256-row batch) on the oracle's batch at the bars of
test_ppo_update_parity, and the tail-row cases also compare the last block's rows of both
branches' W1, and their Adam moments, with the oracle's: a lane -> parameter map that is
wrong, or a parameter left without an owner, shows there first.

Bars for the moments (the file's parameter and statistics bars are test_gpu_parity's): m is a
fixed linear combination of the steps' clipped gradients, so it takes the gradient bar of
test_ddp_grad_and_apply_match_fused_step (rtol 1e-4, atol 2e-5 max |ref|); v is the same
combination of their squares, whose relative error is twice the gradient's (rtol 2e-4,
atol 4e-5 max |ref|).
"""
import numpy as np
import pytest

from oracle import ddrl_oracle as O
from tests import test_gpu_parity as TP
from tests.gpu_harness import filter_state, init_params, make_ctx, run_rollout, strict_params_check

pytestmark = pytest.mark.gpu
STEPS = 4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddrl_amd import build
    build.build()


def _setup(env, n, T, config):
    """Context with the oracle's batch loaded: (ctx, cfg, initial params, oracle rollout, norms)."""
    ctx, cfg, inst = make_ctx(env, n, T, config)
    rng = np.random.default_rng(5)
    params = init_params(ctx, cfg, 7, head_scale=1.0)
    orc, norms, _, _ = run_rollout(ctx, cfg, inst, params, rng, filter_state(cfg.obs_full_dim, rng), T)
    for p in range(cfg.n_policies):
        # feed the ORACLE's batch so the update parity does not inherit rollout rounding
        ctx.records_set(p, orc.flat_records(p, ctx.layout[p]))
        ctx.adv_norm_set(p, *norms[p])
    return ctx, cfg, params, orc, norms


def _tail_slices(d):
    """Flat-vector slices of W1 rows 16 (nf1 - 1) .. d - 1 of the policy and the value branch."""
    f0 = 16 * ((d + 15) // 16 - 1)
    vw1 = d * 64 + 64   # fc_1/kernel [d][64], fc_1/bias [64], fc_value_1/kernel
    return [("fc_1", slice(f0 * 64, d * 64)), ("fc_value_1", slice(vw1 + f0 * 64, vw1 + d * 64))]


CASES = [
    ("QuantrupedMultiEnv_Local", 8, 32, None, 35, 3),
    ("QuantrupedMultiEnv_Local", 8, 32, TP.TVEL, 36, 4),
    ("QuantrupedMultiEnv_FullyDecentral", 8, 32, TP.TVEL, 20, 4),
    ("QuantrupedMultiEnv_SharedDecentral", 8, 8, None, 19, 3),   # one shared policy, 32 rows per step
    ("QuantrupedMultiEnv_SingleNeighbor", 8, 32, None, 27, 11),  # control: 11 rows in the last block
]


@pytest.mark.parametrize("env,n,T,config,d_want,tail", CASES)
def test_update_tail_rows(env, n, T, config, d_want, tail):
    import torch
    ctx, cfg, params, orc, norms = _setup(env, n, T, config)
    shuffles, perms, kls = [], [], []
    for p in range(cfg.n_policies):
        R = T * ctx.layout[p]["C"]
        assert R == 256 and cfg.obs_dim[p] == d_want
        sh, pe = O.sgd_schedule(np.random.default_rng(100 + p), R, 128, cfg.num_sgd_iter)
        shuffles.append(sh)
        perms.append(pe)
        kls.append(0.2 + 0.1 * p)
    dsh = [torch.from_numpy(s).cuda() for s in shuffles]
    dpe = [torch.from_numpy(s).cuda() for s in perms]
    ctx.ppo_update((1 << cfg.n_policies) - 1, dsh, dpe, kls, max_steps=STEPS)
    ctx.synchronize()
    for p in range(cfg.n_policies):
        lay = ctx.layout[p]
        d, A = cfg.obs_dim[p], cfg.act_dim
        assert d - 16 * ((d + 15) // 16 - 1) == tail
        batch = TP._batch_from_records(orc.flat_records(p, lay), lay, d, A, norms[p])
        shapes = O.ffn_param_shapes(d, 2 * A)
        adam = O.Adam(sum(int(np.prod(s)) for _, s in shapes), lr=cfg.lr)
        new, stats = O.ppo_update("ffn", params[p], shapes, adam, batch, shuffles[p], perms[p],
                                  np.float32(kls[p]), {"entropy_coeff": 0.0}, steps=STEPS)
        got, ref, init = ctx.params_get(p), O.pack(new, shapes), O.pack(params[p], shapes)
        TP._params_close(got, ref, cfg.lr, STEPS, f"{env} p{p}")
        strict_params_check(got, "ffn", params[p], shapes, batch, shuffles[p], perms[p], kls[p], STEPS,
                            lr=cfg.lr, msg=f"{env} p{p}")
        m, v, b1p, b2p = ctx.adam_get(p)
        assert b1p == np.float32(adam.b1p) and b2p == np.float32(adam.b2p)
        st = ctx.ppo_stats(p, STEPS)
        for k, s in enumerate(stats):
            want = [s["total_loss"], s["policy_loss"], s["vf_loss"], s["kl"], s["entropy"],
                    s["vf_explained_var"], s["grad_gnorm"]]
            TP._close(st[k, :7], np.array(want, np.float32), rtol=1e-4, atol=1e-5, msg=f"stats step {k}")
        if tail > 4:
            continue
        for name, sl in _tail_slices(d):
            msg = f"{env} p{p} {name} tail rows"
            dm, dv = np.abs(m[sl] - adam.m[sl]).max(), np.abs(v[sl] - adam.v[sl]).max()
            print(f"\n{msg} max |theta - ref| {np.abs(got[sl] - ref[sl]).max():.3g}, |m - ref| {dm:.3g} "
                  f"(max |m| {np.abs(adam.m).max():.3g}), |v - ref| {dv:.3g} (max |v| {np.abs(adam.v).max():.3g})")
            TP._params_close(got[sl], ref[sl], cfg.lr, STEPS, msg)
            np.testing.assert_allclose(m[sl], adam.m[sl], rtol=1e-4, atol=2e-5 * np.abs(adam.m).max(), err_msg=msg + " m")
            np.testing.assert_allclose(v[sl], adam.v[sl], rtol=2e-4, atol=4e-5 * np.abs(adam.v).max(), err_msg=msg + " v")
            # every tail parameter has an owner that stepped it
            assert np.all(got[sl] != init[sl]), msg + ": parameters left at their initial values"
            assert np.all(m[sl] != 0) and np.all(v[sl] != 0), msg + ": moments left at zero"
    ctx.close()


def test_grad_export_tail_rows():
    """ddrl_ppo_grad at d = 35: the exported gradient, its last W1 block's rows included, matches
    the oracle at the bar of test_ddp_grad_and_apply_match_fused_step."""
    import torch
    ctx, cfg, params, orc, norms = _setup("QuantrupedMultiEnv_Local", 8, 32, None)
    p, d, A = 1, 35, cfg.act_dim
    lay = ctx.layout[p]
    rows = np.random.default_rng(3).permutation(32 * lay["C"])[:128].astype(np.int32)
    g = torch.zeros(ctx.n_params[p], device="cuda")
    ctx.ppo_grad(p, torch.from_numpy(rows).cuda(), 128, 0.2, g)
    ctx.synchronize()
    gf = g.cpu().numpy()
    batch = TP._batch_from_records(orc.flat_records(p, lay), lay, d, A, norms[p])
    sl = {k: v[rows] for k, v in batch.items()}
    logits, value, cache = O.ffn_forward(params[p], sl["obs"])
    dl, dv, _ = O.ppo_loss_rows(logits, value, sl["actions"], sl["logits"], sl["logp"],
                                sl["vf_preds"], sl["adv"], sl["vt"], np.float32(0.2))
    gref = O.pack(O.ffn_backward(params[p], cache, dl, dv), O.ffn_param_shapes(d, 2 * A))
    atol = 2e-5 * np.abs(gref).max()
    np.testing.assert_allclose(gf, gref, rtol=1e-4, atol=atol)
    for name, s in _tail_slices(d):
        print(f"\n{name} tail rows: max |g - ref| {np.abs(gf[s] - gref[s]).max():.3g}, max |ref| {np.abs(gref[s]).max():.3g}")
        np.testing.assert_allclose(gf[s], gref[s], rtol=1e-4, atol=atol, err_msg=name)
        assert np.all(gf[s] != 0), name + ": tail rows not exported"
    ctx.close()
