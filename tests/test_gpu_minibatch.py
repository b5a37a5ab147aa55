"""sgd_minibatch_size = 256 through the fused persistent update (ppo_ffn_mb256.hip), against the
CPU oracle and against the properties the 128-row path has (needs an MI355X).

Each of a branch's two workgroups takes 128 rows of the minibatch, two 16-row tiles per wave.
The shapes are the smallest that reach both row halves, both tiles of a wave, a second
minibatch slot, an epoch boundary (step nb) and a dropped remainder (R mod 256 != 0).
Criteria are those of tests/test_gpu_parity.py, unchanged: strict_params_check with its default
exemption cap, parameters within 1e-5 of the numpy fp32 oracle, bit-equal beta powers, per-step
statistics at rtol 1e-4 / atol 1e-5.  The numpy-vs-fp64 half of strict_params_check was run on
the CPU for every case below before the seeds were fixed: the reference alone needs no exemption
(0 entries beyond 1e-5 in every case).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ddrl_amd import native as N
from oracle import ddrl_oracle as O
from tests.gpu_harness import (CUP_CONFIG, CUP_ENV, CupOracleRollout, filter_state, init_cup_params, init_params,
                               make_ctx, run_rollout, strict_params_check)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = 256
MBCFG = {"sgd_minibatch_size": MB}
TVEL = {"env_config": {"target_velocity": [1.0]}}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddrl_amd import build
    build.build()


def _close(a, b, rtol=1e-5, atol=1e-5, msg=""):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=msg)


# copies of test_gpu_parity.py's private helpers (+ the "cup" model's leg column)
def _batch_from_records(rec, lay, d, A, adv_norm):
    mean, den = adv_norm
    b = dict(obs=rec[:, lay["obs"]:lay["obs"] + d], actions=rec[:, lay["act"]:lay["act"] + A],
             logits=rec[:, lay["logit"]:lay["logit"] + 2 * A], logp=rec[:, lay["logp"]],
             vf_preds=rec[:, lay["vf"]], adv=((rec[:, lay["adv"]] - mean) / den).astype(np.float32),
             vt=rec[:, lay["vt"]])
    if lay.get("leg", -1) >= 0:
        b["leg"] = rec[:, lay["leg"]].astype(np.int64)
    return b


def _params_close(got, ref, lr, steps, msg):
    diff = np.abs(got - ref)
    frac = np.mean(diff <= 1e-5 + 1e-5 * np.abs(ref))
    assert frac >= 0.999, f"{msg}: only {frac:.5f} of params within 1e-5 (max {diff.max():.3g})"
    assert diff.max() <= 2 * lr * steps + 1e-5, f"{msg}: max deviation {diff.max():.3g}"


def _ctx(env, n, T, config=None, **envvars):
    """A sgd_minibatch_size = 256 context, created under the given environment variables."""
    old = {k: os.environ.get(k) for k in envvars}
    os.environ.update({k: str(v) for k, v in envvars.items()})
    try:
        return make_ctx(env, n, T, {**MBCFG, **(config or {})})
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# env, envs, T, steps, config, model.  R rows per policy -> nb = R // 256, R - 256 nb rows dropped
UPDATE_CASES = [
    ("QuantrupedMultiEnv_Local", 72, 8, 3, None, "ffn"),                # R 576: nb 2, 64 dropped; d 35, KS1 9
    ("QuantrupedMultiEnv_SharedDecentral", 40, 4, 3, None, "ffn"),      # R 640: nb 2, 128 dropped; d 19, KS1 5
    ("QuantrupedMultiEnv_SharedDecentralLegID", 40, 4, 3, None, "ffn"),  # d 23: the generic KS1 12 instance
    ("QuantrupedMultiEnv_TwoSides", 72, 4, 3, None, "ffn"),             # A 4, d 27: R 576, 2 policies
    ("QuantrupedMultiEnv_Local", 66, 4, 2, TVEL, "ffn"),                # d 36 (TVel): R 264, nb 1, 8 dropped
    (CUP_ENV, 40, 4, 3, CUP_CONFIG, "cup"),                             # coupling table on both row halves
    ("QuantrupedMultiEnv_Centralized", 1, 520, 3, None, "ffn"),         # A 8, d 43: one env, R 520, 8 dropped
]


def run_update_case(env, n, T, steps, config, model):
    """Fused 256-row steps of every policy against the oracle (test_gpu_parity.py's pattern)."""
    import torch
    ctx, cfg, inst = _ctx(env, n, T, config)
    assert cfg.sgd_minibatch_size == MB
    cup = model == "cup"
    rng = np.random.default_rng(5)
    params = init_cup_params(ctx, cfg, 7, head_scale=1.0) if cup else init_params(ctx, cfg, 7, head_scale=1.0)
    orc, norms, _, _ = run_rollout(ctx, cfg, inst, params, rng, filter_state(cfg.obs_full_dim, rng), T,
                                   orc_cls=CupOracleRollout if cup else None)
    shuffles, perms, kls = [], [], []
    for p in range(cfg.n_policies):
        lay = ctx.layout[p]
        ctx.records_set(p, orc.flat_records(p, lay))
        ctx.adv_norm_set(p, *norms[p])
        sh, pe = O.sgd_schedule(np.random.default_rng(100 + p), T * lay["C"], MB, cfg.num_sgd_iter)
        assert pe.shape[1] == (T * lay["C"]) // MB
        shuffles.append(sh)
        perms.append(pe)
        kls.append(0.2 + 0.1 * p)
    dsh = [torch.from_numpy(s).cuda() for s in shuffles]
    dpe = [torch.from_numpy(s).cuda() for s in perms]
    ctx.ppo_update((1 << cfg.n_policies) - 1, dsh, dpe, kls, max_steps=steps)
    ctx.synchronize()
    for p in range(cfg.n_policies):
        lay = ctx.layout[p]
        d, A = cfg.obs_dim[p], cfg.act_dim
        batch = _batch_from_records(orc.flat_records(p, lay), lay, d, A, norms[p])
        shapes = O.cup_param_shapes(d, A) if cup else O.ffn_param_shapes(d, 2 * A)
        adam = O.Adam(sum(int(np.prod(s)) for _, s in shapes), lr=cfg.lr)
        new, stats = O.ppo_update(model, params[p], shapes, adam, batch, shuffles[p], perms[p],
                                  np.float32(kls[p]), {"entropy_coeff": 0.0, **MBCFG}, steps=steps)
        got = ctx.params_get(p)
        _params_close(got, O.pack(new, shapes), cfg.lr, steps, f"{env} p{p}")
        strict_params_check(got, model, params[p], shapes, batch, shuffles[p], perms[p], kls[p], steps,
                            cfg=MBCFG, lr=cfg.lr, msg=f"{env} p{p} mb256")
        m, v, b1p, b2p = ctx.adam_get(p)
        assert b1p == np.float32(adam.b1p) and b2p == np.float32(adam.b2p)
        st = ctx.ppo_stats(p, steps)
        for k, s in enumerate(stats):
            ref = [s["total_loss"], s["policy_loss"], s["vf_loss"], s["kl"], s["entropy"],
                   s["vf_explained_var"], s["grad_gnorm"]]
            _close(st[k, :7], np.array(ref, np.float32), rtol=1e-4, atol=1e-5, msg=f"stats step {k}")
    ctx.close()


@pytest.mark.parametrize("env,n,T,steps,config,model", UPDATE_CASES)
def test_ppo_update_parity_mb256(env, n, T, steps, config, model):
    run_update_case(env, n, T, steps, config, model)


def test_full_schedule_mb256():
    """Local 64 x 8 (R = 512, nb = 2): the whole 10-epoch schedule, 20 steps of 256 rows."""
    import torch
    env, n, T = "QuantrupedMultiEnv_Local", 64, 8
    ctx, cfg, inst = _ctx(env, n, T)
    rng = np.random.default_rng(9)
    params = init_params(ctx, cfg, 2, head_scale=1.0)
    orc, norms, _, _ = run_rollout(ctx, cfg, inst, params, rng, filter_state(cfg.obs_full_dim, rng), T)
    sh, pe = O.sgd_schedule(np.random.default_rng(1), T * n, MB, 10)
    assert pe.shape == (10, 2)
    for p in range(4):
        ctx.records_set(p, orc.flat_records(p, ctx.layout[p]))
        ctx.adv_norm_set(p, *norms[p])
    dsh = [torch.from_numpy(sh).cuda()] * 4
    dpe = [torch.from_numpy(pe).cuda()] * 4
    ctx.ppo_update(0xF, dsh, dpe, [0.2] * 4)
    ctx.synchronize()
    p = 1
    lay = ctx.layout[p]
    batch = _batch_from_records(orc.flat_records(p, lay), lay, 35, 2, norms[p])
    shapes = O.ffn_param_shapes(35, 4)
    adam = O.Adam(sum(int(np.prod(s)) for _, s in shapes))
    new, stats = O.ppo_update("ffn", params[p], shapes, adam, batch, sh, pe, np.float32(0.2), dict(MBCFG))
    assert len(stats) == 20
    got = ctx.params_get(p)
    assert np.abs(got - O.pack(new, shapes)).max() <= 1e-5
    strict_params_check(got, "ffn", params[p], shapes, batch, sh, pe, 0.2, 20, cfg=MBCFG, msg="full schedule mb256")
    st = ctx.ppo_stats(p, 20)
    _close(st[-1, 0], stats[-1]["total_loss"], rtol=1e-3, atol=1e-4)
    np.testing.assert_array_equal(ctx.ppo_stats(p, 2, first=18), st[18:])
    with pytest.raises(N.DdrlError):
        ctx.ppo_stats(p, 3, first=18)              # past the 10 x 2 schedule
    ctx.close()


def test_two_128_row_gradients_and_apply_match_fused_step_mb256():
    """ddrl_ppo_grad stays at <= 128 rows and scales by 1 / sgd_minibatch_size: on a 256 context
    the gradients of the two halves of a minibatch sum to its gradient, and apply == fused step."""
    import torch
    env, n, T = "QuantrupedMultiEnv_SharedDecentral", 32, 4   # R = 512
    ctx, cfg, inst = _ctx(env, n, T)
    rng = np.random.default_rng(4)
    params = init_params(ctx, cfg, 8, head_scale=1.0)
    orc, norms, _, _ = run_rollout(ctx, cfg, inst, params, rng, filter_state(cfg.obs_full_dim, rng), T)
    lay = ctx.layout[0]
    ctx.records_set(0, orc.flat_records(0, lay))
    ctx.adv_norm_set(0, *norms[0])
    R = T * lay["C"]
    rows = np.random.default_rng(3).permutation(R)[:MB].astype(np.int32)
    npar = ctx.n_params[0]
    g_a = torch.zeros(npar, device="cuda")
    g_b = torch.zeros(npar, device="cuda")
    r_all = torch.from_numpy(rows).cuda()
    ctx.ppo_grad(0, r_all[:128].contiguous(), 128, 0.2, g_a)
    ctx.ppo_grad(0, r_all[128:].contiguous(), 128, 0.2, g_b)
    with pytest.raises(N.DdrlError):
        ctx.ppo_grad(0, r_all, MB, 0.2, g_a)     # a gradient launch carries at most 128 rows
    ctx.synchronize()
    g_sum = g_a + g_b
    gs = g_sum.cpu().numpy()
    # oracle gradient of the 256 rows (means over 256)
    batch = _batch_from_records(orc.flat_records(0, lay), lay, 19, 2, norms[0])
    sl = {k: v[rows] for k, v in batch.items()}
    logits, value, cache = O.ffn_forward(params[0], sl["obs"])
    dl, dv, _ = O.ppo_loss_rows(logits, value, sl["actions"], sl["logits"], sl["logp"],
                                sl["vf_preds"], sl["adv"], sl["vt"], np.float32(0.2))
    shapes = O.ffn_param_shapes(19, 4)
    gref = O.pack(O.ffn_backward(params[0], cache, dl, dv), shapes)
    np.testing.assert_allclose(gs, gref, rtol=1e-4, atol=2e-5 * np.abs(gref).max())
    theta0 = ctx.params_get(0)
    ctx.ppo_apply(0, g_sum)
    ctx.synchronize()
    got = ctx.params_get(0)
    adam = O.Adam(npar)
    clipped, _ = O.clip_by_global_norm([gref], 0.5)
    _params_close(got, adam.apply(O.pack(params[0], shapes), clipped[0]), 3e-4, 1, "ddp apply mb256")
    # the same step as a one-step schedule whose first minibatch is `rows`: against fp64 ...
    rest = np.setdiff1d(np.arange(R, dtype=np.int32), rows)
    sh1 = np.concatenate([rows, rest]).astype(np.int32)
    pe1 = np.arange(R // MB, dtype=np.int32)[None]
    strict_params_check(got, "ffn", params[0], shapes, batch, sh1, pe1, 0.2, 1, cfg=MBCFG, msg="ddp apply mb256")
    # ... and against the fused kernel's step from the same state
    ctx.params_set(0, theta0)
    ctx.adam_set(0, np.zeros(npar, np.float32), np.zeros(npar, np.float32), 0.9, 0.999)
    ctx.ppo_update(1, [torch.from_numpy(sh1).cuda()], [torch.from_numpy(pe1).cuda()], [0.2], max_steps=1)
    ctx.synchronize()
    _params_close(got, ctx.params_get(0), 3e-4, 1, "ddp apply vs fused step mb256")
    ctx.close()


# ---- properties of the launch: resume, protocols, rollback (a seeded device rollout, no oracle) ----
def _prepared(env="QuantrupedMultiEnv_Local", n=64, T=8, **envvars):
    import torch
    from ddrl_amd.synthetic import SyntheticRollout
    ctx, cfg, _ = _ctx(env, n, T, **envvars)
    init_params(ctx, cfg, 3, head_scale=1.0)
    syn = SyntheticRollout(n, T, cfg.obs_full_dim, cfg.n_agents, cfg.act_dim, "cuda:0", seed=5)
    ctx.observe(syn.obs[0])
    ctx.rollout_fragment(syn.obs, syn.eps, syn.fw, syn.cfrc, syn.dones_for_fragment(), syn.actions)
    ctx.gae()
    ctx.synchronize()
    rng = np.random.default_rng(9)
    sh, pe = [], []
    for p in range(cfg.n_policies):
        s, q = O.sgd_schedule(rng, T * ctx.layout[p]["C"], MB, cfg.num_sgd_iter)
        sh.append(torch.from_numpy(s).cuda())
        pe.append(torch.from_numpy(q).cuda())
    return ctx, cfg, sh, pe


def _state(ctx, P, H=0):
    out = []
    for p in range(P):
        m, v, b1, b2 = ctx.adam_get(p)
        out += [ctx.params_get(p), m, v, np.array([b1, b2], np.float32)] + ([ctx.ppo_stats(p, H)] if H else [])
    return out


def _reset(ctx, theta0):
    for p, th in enumerate(theta0):
        ctx.params_set(p, th)
        ctx.adam_set(p, np.zeros(th.size, np.float32), np.zeros(th.size, np.float32), 0.9, 0.999)


def test_resumed_update_is_bit_identical_mb256():
    """7 steps as 1 + 2 + 4 (launches starting at steps 0, 1 and 3: both outbox parities and both
    values of the quads' tag bit as a launch's first) equal one launch, bit for bit."""
    ctx, cfg, sh, pe = _prepared()
    P = cfg.n_policies
    mask, kl = (1 << P) - 1, [0.2] * P
    theta0 = [ctx.params_get(p) for p in range(P)]
    ctx.ppo_update(mask, sh, pe, kl, max_steps=7)
    ctx.synchronize()
    ref = _state(ctx, P, 7)
    _reset(ctx, theta0)
    ctx.ppo_update(mask, sh, pe, kl, max_steps=1)
    ctx.ppo_update(mask, sh, pe, kl, max_steps=2, step0=1)
    ctx.ppo_update(mask, sh, pe, kl, max_steps=4, step0=3)
    ctx.synchronize()
    for i, (a, b) in enumerate(zip(_state(ctx, P, 7), ref)):
        np.testing.assert_array_equal(a, b, err_msg=f"1 + 2 + 4 steps, item {i}")
    assert not np.array_equal(ref[0], theta0[0]) and np.isfinite(ref[4]).all()
    ctx.close()


def test_atomic_exchange_matches_default_protocol_bit_for_bit_mb256():
    res = []
    for env in ({}, {"DDRL_XCHG": "atomic"}):
        ctx, cfg, sh, pe = _prepared(**env)
        P = cfg.n_policies
        ctx.ppo_update((1 << P) - 1, sh, pe, [0.2] * P)   # the whole schedule: 10 epochs x 2 = 20 steps
        ctx.synchronize()
        res.append(_state(ctx, P, 20))
        ctx.close()
    assert np.isfinite(res[0][0]).all() and np.isfinite(res[0][4]).all()
    for i, (x, y) in enumerate(zip(*res)):
        np.testing.assert_array_equal(x, y, err_msg=f"item {i}")


def test_failed_update_leaves_state_unchanged_mb256():
    ctx, cfg, sh, pe = _prepared(DDRL_TEST_FAIL_STEP=5)
    P = cfg.n_policies
    ctx.adam_set(0, *[np.full(ctx.n_params[0], 1e-3, np.float32)] * 2, 0.9 ** 3, 0.999 ** 3)
    before = _state(ctx, P)
    ctx.ppo_update((1 << P) - 1, sh, pe, [0.2] * P)
    with pytest.raises(N.DdrlError, match="as before the call"):
        ctx.ppo_stats(0, 4)
    for i, (b, a) in enumerate(zip(before, _state(ctx, P))):
        np.testing.assert_array_equal(a, b, err_msg=f"item {i}")
    ctx.close()


def test_refusals_name_sgd_minibatch_size():
    import torch
    # one workgroup per branch cannot hold 256-row images: refused when the context is made
    with pytest.raises(N.DdrlError, match="sgd_minibatch_size"):
        _ctx("QuantrupedMultiEnv_Local", 64, 8, DDRL_UPDATE_SPLIT=1)
    # peer mode splits a 128-row minibatch over two ranks
    ctx, cfg, _ = _ctx("QuantrupedMultiEnv_SharedDecentral", 32, 4)
    gx, _ = ctx.peer_alloc()
    with pytest.raises(N.DdrlError, match="sgd_minibatch_size"):
        ctx.peer_attach(gx, 0)
    sh = torch.zeros(64 * 8, dtype=torch.int32, device="cuda")
    pe = torch.zeros((cfg.num_sgd_iter, 8), dtype=torch.int32, device="cuda")
    with pytest.raises(N.DdrlError, match="no peer"):
        ctx.ppo_update_peer(0, sh, pe, 0.2)
    ctx.close()
    # a train batch of fewer rows than one minibatch: 30 envs x T 8 = 240 rows per leg policy
    ctx, cfg, _ = _ctx("QuantrupedMultiEnv_Local", 30, 8)
    theta0 = ctx.params_get(0)
    sh = [torch.zeros(240, dtype=torch.int32, device="cuda") for _ in range(4)]
    pe = [torch.zeros((cfg.num_sgd_iter, 1), dtype=torch.int32, device="cuda") for _ in range(4)]
    with pytest.raises(N.DdrlError, match="sgd_minibatch_size 256"):
        ctx.ppo_update(0xF, sh, pe, [0.2] * 4)
    ctx.synchronize()
    np.testing.assert_array_equal(ctx.params_get(0), theta0)
    ctx.close()


def test_update_kernel_indices_in_bounds_mb256():
    """The Local and A = 4 parity cases under the bounds-checked library (tools/bounds_check.py
    --minibatch 256, a child process that loads libddrl_hip_bounds.so): parity green, every counter 0."""
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tools", "bounds_check.py"), "--minibatch", "256"],
                       capture_output=True, text=True, timeout=110, cwd=ROOT)
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert lines and lines[-1].get("bounds_check") == "ok", r.stdout[-4000:] + r.stderr[-4000:]
    cases = lines[:-1]
    assert len(cases) == lines[-1]["cases"] == 2
    assert any("Local" in c["case"] for c in cases) and any("TwoSides" in c["case"] for c in cases)
    for c in cases:
        assert c["status"] == "pass" and not any(c["violations"].values()), c
    assert r.returncode == 0


def test_trainer_two_iterations_mb256():
    from ddrl_amd.trainer import PPOTrainer, update_kl
    T, n = 64, 8
    tr = PPOTrainer({"env": "QuantrupedMultiEnv_Local", "rollout_fragment_length": T, **MBCFG}, n_envs=n, seed=3)
    assert tr.cfg.sgd_minibatch_size == MB
    nb = T * n // MB                      # one leg per policy: R = 512 rows, nb = 2
    E = tr.cfg.num_sgd_iter
    coeff = list(tr.kl_coeff)
    for it in range(2):
        r = tr.train()
        assert r["timesteps_total"] == (it + 1) * T * n
        for p, pid in enumerate(tr.policy_ids):
            st = r["info"]["learner"][pid]
            for k in ("total_loss", "policy_loss", "vf_loss", "kl", "entropy", "vf_explained_var"):
                assert np.isfinite(st[k]), (pid, k)
            last = tr.ctx.ppo_stats(p, nb, first=(E - 1) * nb)
            assert st["kl"] == last[:, 3].astype(np.float64).mean()
            assert st["cur_kl_coeff"] == float(np.float32(coeff[p]))
            coeff[p] = update_kl(coeff[p], st["kl"], tr.config["kl_target"])
            assert tr.kl_coeff[p] == coeff[p]
    tr.stop()
