"""The PPO update kernels away from the default hyperparameters, against the CPU oracle (needs an
MI355X).

Every other update test runs at clip_param 0.2, vf_clip_param 10, vf_loss_coeff 0.5,
entropy_coeff 0, grad_clip 0.5, the ray10 value clip and a positive kl_coeff, on records that
come from the parameters the update starts at.  There the entropy term is multiplied by zero, the
squared value clip and the unclipped global-norm branch never run, and no clip decision is near
its threshold.  This file runs every instance of the update (the fused row-split kernel at three
shapes, the atomic exchange, the split-less kernel, the 256-row kernels in both protocols, the
cup model, GraphNet under both tails, gradient export + apply) under the sets
tests/gpu_harness.HYPER_SETS:

  H1  entropy_coeff 0.01
  H2  entropy_coeff 0.01, clip_param 0.1, vf_clip_param 0.5, vf_loss_coeff 1.0
  H3  vf_clip_mode "squared", vf_clip_param 1.0, clip_param 0.3, entropy_coeff -0.005
  H4  grad_clip None, lr 1e-3
  H5  grad_clip 40.0, kl_coeff 0.0 passed to the update
  H6  grad_clip 0.05, lr 1e-4

on a host-built batch whose rows straddle every clip decision (gpu_harness.StraddlingBatch).
Preconditions, asserted on the reference before the device is looked at: every side of every
clip decision of the case's mode holds >= 5 % of the first minibatch; every step's gradient norm
is below the clip under H4 and H5 and above it under H6 and the default, so both outcomes of the
clip scale's min run.

Bars are the project's own, none new: test_gpu_parity's _params_close, strict_params_check with
its default exemption cap, bit-equal beta powers, the seven statistics columns at rtol 1e-4 /
atol 1e-5 (total_loss is the host's combination with vf_loss_coeff and entropy_coeff); Adam's m
and v at the bars test_gpu_update_tail.py derives (rtol 1e-4 / 2e-4, atol 2e-5 / 4e-5 of
max |ref|); gradients at the bar of test_ddp_grad_and_apply_match_fused_step.  The numpy fp32
oracle alone meets strict_params_check in every case below with no entry beyond 1e-5 (run on the
CPU before the seeds were fixed), so a failure is the kernel's.
"""
import functools

import numpy as np
import pytest

from ddrl_amd.spec import make_cfg
from oracle import ddrl_oracle as O
from tests.gpu_harness import (CUP_CONFIG, CUP_ENV, GNN_ENV, HYPER_SETS, StraddlingBatch, assert_branch_floor, branch_shares,
                               make_ctx,
                               make_model_params, model_shapes, strict_params_check)

pytestmark = pytest.mark.gpu
SHARED = ("QuantrupedMultiEnv_SharedDecentral", 32, 4)     # R = 512, d = 19, A = 2
CENTRAL = ("QuantrupedMultiEnv_Centralized", 64, 4)        # R = 256, d = 43, A = 8
LOCAL = ("QuantrupedMultiEnv_Local", 64, 4)                # four policies in one launch, d = 35
CUP = (CUP_ENV, 32, 4)                                     # R = 512
GNN = (GNN_ENV, 16, 4)                                     # R = 256
MODEL_CONFIG = {"ffn": {}, "cup": CUP_CONFIG, "gnn": {}}
# The Centralized env's one agent pays all four legs' control and contact costs: at the default
# weights every |V - value target| of its synthetic batch is above 1.4, at any seed and size tried
# (64 x 4, 128 x 2, 256 x 1 rows), so H3's squared clip at vf_clip_param 1.0 would have no row inside.
# A tenth of the cost weights brings the targets to the other shapes' scale; d, A, the kernel
# instance, the hyperparameter sets and the 5 % floor are unchanged.
ENV_CONFIG = {CENTRAL[0]: {"env_config": {"ctrl_cost_weight": 0.05, "contact_cost_weight": 5e-3}}}
# The perturbation seed is 11 except at the Local shape: there seed 11 puts one row's ratio within
# 1.9e-7 (relative) of 1 + clip_param under H3 at step 0 of policy 3 -- below fp32 resolution of the
# ratio, so the rounding picks the surrogate's branch (numpy fp32 took fp64's side, the kernel the
# other; the two gradients differ by that row alone).  With the seeds below the smallest margin of
# any clip decision along the fp64 trajectories of this file's cases is 2e-5.
PERTURB_SEED = {LOCAL[0]: 16}
STAT_KEYS = ("total_loss", "policy_loss", "vf_loss", "kl", "entropy", "vf_explained_var", "grad_gnorm")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddrl_amd import build
    build.build()


def _params_close(got, ref, lr, steps, msg):
    diff = np.abs(got - ref)
    frac = np.mean(diff <= 1e-5 + 1e-5 * np.abs(ref))
    assert frac >= 0.999, f"{msg}: only {frac:.5f} of params within 1e-5 (max {diff.max():.3g})"
    assert diff.max() <= 2 * lr * steps + 1e-5, f"{msg}: max deviation {diff.max():.3g}"


def _config(env, model, hyper, mb):
    cfg = {**ENV_CONFIG.get(env, {}), **MODEL_CONFIG[model], **HYPER_SETS.get(hyper, {}), "sgd_minibatch_size": mb}
    cfg.pop("kl_coeff", None)      # passed to the update, not a field of the context
    return cfg


def _oracle_cfg(hyper, mb):
    return {"entropy_coeff": 0.0, **HYPER_SETS.get(hyper, {}), "sgd_minibatch_size": mb}


def _kl(hyper, p):
    return HYPER_SETS.get(hyper, {}).get("kl_coeff", 0.2 + 0.1 * p)


@functools.lru_cache(maxsize=None)
def host_case(env, n, T, model, hyper, mb):
    """(cfg, starting parameters, StraddlingBatch) of a case, built on the host once and shared,
    unchanged, by the instances that run it."""
    cfg, inst = make_cfg(env, n, T, _config(env, model, hyper, mb))
    params = make_model_params(cfg, model, 7)
    return cfg, params, StraddlingBatch(cfg, inst, params, model, HYPER_SETS.get(hyper, {}),
                                        seed=PERTURB_SEED.get(env, 11), mb=mb)


@functools.lru_cache(maxsize=None)
def reference(env, n, T, model, hyper, mb, steps):
    """The numpy fp32 oracle's `steps` steps of every policy: [(theta, stats, m, v, b1p, b2p)]."""
    cfg, params, sb = host_case(env, n, T, model, hyper, mb)
    out = []
    for p in range(cfg.n_policies):
        shapes = model_shapes(cfg, model, p)
        adam = O.Adam(sum(int(np.prod(s)) for _, s in shapes), lr=cfg.lr)
        new, stats = O.ppo_update(model, params[p], shapes, adam, sb.batches[p], sb.shuffles[p], sb.perms[p],
                                  np.float32(_kl(hyper, p)), _oracle_cfg(hyper, mb), steps=steps)
        assert len(stats) == steps
        out.append((O.pack(new, shapes), stats, adam.m, adam.v, adam.b1p, adam.b2p))
    return out


def check_preconditions(env, n, T, model, hyper, mb, steps):
    """On the reference alone: the branch shares' floor, and the side of the clip every step's
    gradient norm is on."""
    cfg, params, sb = host_case(env, n, T, model, hyper, mb)
    ref = reference(env, n, T, model, hyper, mb, steps)
    H = HYPER_SETS.get(hyper, {})
    clip = O.grad_clip_value(H.get("grad_clip", 0.5))
    for p in range(cfg.n_policies):
        gn = [s["grad_gnorm"] for s in ref[p][1]]
        print(f"\n{env} {model} {hyper} mb{mb} p{p}: first-minibatch branch shares "
              + ", ".join(f"{k} {v:.0%}" for k, v in sb.shares[p].items())
              + f"; gradient norms {min(gn):.3g} .. {max(gn):.3g} against a clip of {clip:g}")
        assert_branch_floor(sb.shares[p], f"{env} {hyper} p{p}")
        assert np.all(np.isfinite(gn))
        if hyper in ("H4", "H5"):
            assert max(gn) < clip, (hyper, gn, clip)        # never clipped: min picks 1 / grad_clip
        elif hyper in ("H6", "default"):
            assert min(gn) > clip, (hyper, gn, clip)        # always clipped: min picks 1 / norm


def _make_ctx(env, n, T, config, envvars):
    """A context made under the given environment variables (read when the context is made)."""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in (envvars or {}).items():
            mp.setenv(k, str(v))
        return make_ctx(env, n, T, config)


def _load(ctx, cfg, model, params, sb):
    for p in range(cfg.n_policies):
        lay = ctx.layout[p]
        ctx.params_set(p, O.pack(params[p], model_shapes(cfg, model, p)))
        rec = sb.records(p, lay)
        b = sb.batches[p]
        # the device and the oracle read the same perturbed rows
        assert np.array_equal(rec[:, lay["logp"]], b["logp"]) and np.array_equal(rec[:, lay["vf"]], b["vf_preds"])
        assert np.array_equal(rec[:, lay["vt"]], b["vt"])
        ctx.records_set(p, rec)
        ctx.adv_norm_set(p, *sb.norms[p])


def run_update_case(shape, steps, hyper, model="ffn", mb=128, envvars=None):
    """test_gpu_parity.test_ppo_update_parity's body under a hyperparameter set, on the straddling
    batch, plus Adam's moments."""
    import torch
    env, n, T = shape
    check_preconditions(env, n, T, model, hyper, mb, steps)
    _, params, sb = host_case(env, n, T, model, hyper, mb)
    ref = reference(env, n, T, model, hyper, mb, steps)
    ctx, cfg, _ = _make_ctx(env, n, T, _config(env, model, hyper, mb), envvars)
    assert cfg.sgd_minibatch_size == mb
    _load(ctx, cfg, model, params, sb)
    P = cfg.n_policies
    kls = [_kl(hyper, p) for p in range(P)]
    dsh = [torch.from_numpy(s).cuda() for s in sb.shuffles]
    dpe = [torch.from_numpy(s).cuda() for s in sb.perms]
    ctx.ppo_update((1 << P) - 1, dsh, dpe, kls, max_steps=steps)
    ctx.synchronize()
    for p in range(P):
        msg = f"{env} {model} {hyper} mb{mb} {envvars or ''} p{p}"
        shapes = model_shapes(cfg, model, p)
        want, stats, m_ref, v_ref, b1p_ref, b2p_ref = ref[p]
        got = ctx.params_get(p)
        _params_close(got, want, cfg.lr, steps, msg)
        strict_params_check(got, model, params[p], shapes, sb.batches[p], sb.shuffles[p], sb.perms[p], kls[p], steps,
                            cfg=_oracle_cfg(hyper, mb), lr=cfg.lr, msg=msg)
        m, v, b1p, b2p = ctx.adam_get(p)
        assert b1p == np.float32(b1p_ref) and b2p == np.float32(b2p_ref)
        np.testing.assert_allclose(m, m_ref, rtol=1e-4, atol=2e-5 * np.abs(m_ref).max(), err_msg=msg + " adam m")
        np.testing.assert_allclose(v, v_ref, rtol=2e-4, atol=4e-5 * np.abs(v_ref).max(), err_msg=msg + " adam v")
        st = ctx.ppo_stats(p, steps)
        for k, s in enumerate(stats):
            np.testing.assert_allclose(st[k, :7], np.array([s[key] for key in STAT_KEYS], np.float32),
                                       rtol=1e-4, atol=1e-5, err_msg=f"{msg} stats step {k}")
        if model == "cup":   # the coupling table's eight entries, as in test_cup_fused_update_parity
            np.testing.assert_allclose(got[-8:], want[-8:], rtol=1e-5, atol=1e-5)
            assert np.abs(got[-8:] - O.pack(params[p], shapes)[-8:]).max() > 0
            assert np.all(v[-8:] > 0), "coupling entries carry Adam state"
    ctx.close()


@pytest.mark.parametrize("hyper", ["default", "H1", "H2", "H3", "H4", "H5", "H6"])
def test_fused_update_under_hyperparameters(hyper):
    """The fused row-split kernel (the default): SharedDecentral, R = 512, 4 steps."""
    run_update_case(SHARED, 4, hyper)


@pytest.mark.parametrize("hyper", ["H2", "H3"])
@pytest.mark.parametrize("shape", [CENTRAL, LOCAL], ids=["Centralized-A8-d43", "Local-4-policies-d35"])
def test_fused_update_other_shapes(shape, hyper):
    run_update_case(shape, 4, hyper)


INSTANCES = [
    pytest.param(128, {"DDRL_XCHG": "atomic"}, id="atomic"),
    pytest.param(128, {"DDRL_UPDATE_SPLIT": 1}, id="split1"),
    pytest.param(256, None, id="mb256"),
    pytest.param(256, {"DDRL_XCHG": "atomic"}, id="mb256-atomic"),
]


@pytest.mark.parametrize("hyper", ["H2", "H3", "H5"])
@pytest.mark.parametrize("mb,envvars", INSTANCES)
def test_other_update_instances(mb, envvars, hyper):
    """The atomic exchange, the split-less kernel and the 256-row kernels in both exchange
    protocols: separate translation units that consume the same UpdateHyper."""
    run_update_case(SHARED, 4, hyper, mb=mb, envvars=envvars)


@pytest.mark.parametrize("hyper", ["H2", "H3"])
def test_cup_update_under_hyperparameters(hyper):
    run_update_case(CUP, 2, hyper, model="cup")


@pytest.mark.parametrize("hyper", ["H2", "H3", "H5"])
@pytest.mark.parametrize("tail", ["1", "0"], ids=["one-launch-tail", "three-launch"])
def test_gnn_update_under_hyperparameters(tail, hyper):
    run_update_case(GNN, 2, hyper, model="gnn", envvars={"DDRL_GNN_TAIL": tail})


@pytest.mark.parametrize("hyper", ["H2", "H3", "H4"])
@pytest.mark.parametrize("model,shape", [("ffn", SHARED), ("gnn", GNN)], ids=["ffn", "gnn"])
def test_grad_export_and_apply_under_hyperparameters(model, shape, hyper):
    """ddrl_ppo_grad of 128 chosen rows against the oracle's gradient, then ddrl_ppo_apply against
    clip_by_global_norm(gradient, the case's clip) + the oracle's Adam."""
    import torch
    env, n, T = shape
    cfg, params, sb = host_case(env, n, T, model, hyper, 128)
    H = HYPER_SETS[hyper]
    b = sb.batches[0]
    R = b["logp"].size
    rows = np.random.default_rng(3).permutation(R)[:128].astype(np.int32)
    sl = {k: v[rows] for k, v in b.items()}
    shapes = model_shapes(cfg, model, 0)
    if model == "gnn":
        logits, value, cache = O.gnn_forward(params[0], sl["X"], sl["node_idx"])
    else:
        logits, value, cache = O.ffn_forward(params[0], sl["obs"])
    loss_kw = {k: H[k] for k in ("clip_param", "vf_clip_param", "vf_loss_coeff", "entropy_coeff", "vf_clip_mode")
               if k in H}
    dl, dv, _ = O.ppo_loss_rows(logits, value, sl["actions"], sl["logits"], sl["logp"], sl["vf_preds"], sl["adv"],
                                sl["vt"], np.float32(0.2), **loss_kw)
    gref = O.pack((O.gnn_backward if model == "gnn" else O.ffn_backward)(params[0], cache, dl, dv), shapes)
    shares = branch_shares(logits, value, sl, H)
    clip = O.grad_clip_value(H.get("grad_clip", 0.5))
    clipped, gn = O.clip_by_global_norm([gref], clip)
    print(f"\n{env} {model} {hyper}: branch shares of the rows " + ", ".join(f"{k} {v:.0%}" for k, v in shares.items())
          + f"; gradient norm {gn:.3g} against a clip of {clip:g}")
    assert_branch_floor(shares, f"{model} {hyper}")
    assert (gn < clip) if hyper == "H4" else (gn > clip), (gn, clip)
    ctx, dcfg, _ = _make_ctx(env, n, T, _config(env, model, hyper, 128), None)
    _load(ctx, dcfg, model, params, sb)
    g = torch.zeros(ctx.n_params[0], device="cuda")
    ctx.ppo_grad(0, torch.from_numpy(rows).cuda(), 128, 0.2, g)
    ctx.synchronize()
    gf = g.cpu().numpy()
    print(f"\n{env} {model} {hyper}: max |g - ref| {np.abs(gf - gref).max():.3g}, max |ref| {np.abs(gref).max():.3g}")
    np.testing.assert_allclose(gf, gref, rtol=1e-4, atol=2e-5 * np.abs(gref).max())
    ctx.ppo_apply(0, g)
    ctx.synchronize()
    want = O.Adam(gref.size, lr=dcfg.lr).apply(O.pack(params[0], shapes), clipped[0])
    got = ctx.params_get(0)
    _params_close(got, want, dcfg.lr, 1, f"{model} {hyper} apply")
    # the same step as a one-step schedule whose first minibatch is `rows`, against fp64
    rest = np.setdiff1d(np.arange(R, dtype=np.int32), rows)
    sh1 = np.concatenate([rows, rest]).astype(np.int32)
    pe1 = np.arange(R // 128, dtype=np.int32)[None]
    strict_params_check(got, model, params[0], shapes, b, sh1, pe1, 0.2, 1, cfg=_oracle_cfg(hyper, 128), lr=dcfg.lr,
                        msg=f"{model} {hyper} apply")
    ctx.close()
