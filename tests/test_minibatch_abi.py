"""CPU checks for sgd_minibatch_size = 256: which sizes ddrl_ctx_create accepts, and the oracle's
schedule and update at 256 rows (the reference the GPU tests of tests/test_gpu_minibatch.py
compare against)."""
import ctypes

import numpy as np
import pytest

from ddrl_amd import build, native
from ddrl_amd.spec import make_cfg
from oracle import ddrl_oracle as O

FFN_ENV = "QuantrupedMultiEnv_Local"
GNN_ENV = "QuantrupedMultiEnv_DecentralShared_Graph"


@pytest.fixture(scope="module")
def lib():
    build.build()
    return native.load()


def _create(lib, env, mb, config=None):
    """ddrl_ctx_create of `env` at sgd_minibatch_size mb -> (rc, ddrl_last_error())."""
    cfg, _ = make_cfg(env, 4, 2, {"sgd_minibatch_size": mb, **(config or {})})
    assert cfg.sgd_minibatch_size == mb
    h = ctypes.c_void_p()
    rc = lib.ddrl_ctx_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    err = lib.ddrl_last_error() if rc else b""
    if rc == 0:
        lib.ddrl_ctx_destroy(h)
    return rc, err


@pytest.mark.parametrize("mb", [64, 192, 512])
def test_other_minibatch_sizes_stay_refused(lib, mb):
    rc, err = _create(lib, FFN_ENV, mb)
    assert rc != 0 and b"sgd_minibatch_size" in err, err


def test_graphnet_stays_at_128(lib):
    rc, err = _create(lib, GNN_ENV, 256)
    assert rc != 0 and b"sgd_minibatch_size" in err and b"GraphNet" in err, err


@pytest.mark.parametrize("env,config", [(FFN_ENV, None),
                                        ("QuantrupedMultiEnv_Centralized", None),
                                        ("QuantrupedMultiEnv_SharedDecentralLegID", {"model": {"custom_model": "cup"}})])
def test_fcnet_accepts_256(lib, env, config):
    """The configuration passes validation.  Without a GPU the create still fails, on its first
    device call and with another message."""
    rc, err = _create(lib, env, 256, config)
    assert b"sgd_minibatch_size" not in err, err
    rc, err = _create(lib, env, 128, config)
    assert b"sgd_minibatch_size" not in err, err


def test_row_split_off_is_refused_at_256(lib, monkeypatch):
    monkeypatch.setenv("DDRL_UPDATE_SPLIT", "1")
    rc, err = _create(lib, FFN_ENV, 256)
    assert rc != 0 and b"sgd_minibatch_size" in err and b"DDRL_UPDATE_SPLIT" in err, err
    rc, err = _create(lib, FFN_ENV, 128)       # the 128-row kernels have the split-less instances
    assert b"sgd_minibatch_size" not in err, err


def _tiny_batch(rng, R, d, A):
    return dict(obs=rng.normal(size=(R, d)).astype(np.float32), actions=rng.normal(size=(R, A)).astype(np.float32),
                logits=(rng.normal(size=(R, 2 * A)) * 0.1).astype(np.float32),
                logp=(rng.normal(size=R) - 2).astype(np.float32), vf_preds=rng.normal(size=R).astype(np.float32),
                adv=rng.normal(size=R).astype(np.float32), vt=rng.normal(size=R).astype(np.float32))


def test_oracle_schedule_and_update_follow_the_row_rule_at_256():
    """nb = R // 256; row i of step (e, b) is shuffle[perm[e][b] * 256 + i]; rows past nb * 256 are
    left out; loss means are over 256 rows."""
    R, d, A, mb, E = 600, 19, 2, 256, 3
    sh, pe = O.sgd_schedule(np.random.default_rng(3), R, mb, E)
    assert sh.shape == (R,) and sorted(sh) == list(range(R)) and pe.shape == (E, R // mb) == (3, 2)
    for e in range(E):
        assert sorted(pe[e]) == [0, 1]
        for b in range(2):
            rows = O.minibatch_rows(sh, pe, e, b, mb)
            np.testing.assert_array_equal(rows, [sh[pe[e][b] * mb + i] for i in range(mb)])
    used = {int(r) for e in range(E) for b in range(2) for r in O.minibatch_rows(sh, pe, e, b, mb)}
    assert used == set(sh[:2 * mb].tolist()) and len(used) == 2 * mb     # 88 rows never train
    rng = np.random.default_rng(4)
    batch = _tiny_batch(rng, R, d, A)
    params = O.ffn_init(rng, d, 2 * A)
    shapes = O.ffn_param_shapes(d, 2 * A)
    n = sum(int(np.prod(s)) for _, s in shapes)
    cfg = {"entropy_coeff": 0.0, "sgd_minibatch_size": mb}
    glog = []
    new, stats = O.ppo_update("ffn", params, shapes, O.Adam(n), batch, sh, pe, np.float32(0.2), cfg, steps=3,
                              gradlog=glog)
    assert len(stats) == len(glog) == 3    # step 2 is the first minibatch of epoch 1
    # step 0 by hand: forward, loss and gradient of the rule's 256 rows, clip, Adam
    rows = sh[pe[0][0] * mb:pe[0][0] * mb + mb]
    sl = {k: v[rows] for k, v in batch.items()}
    logits, value, cache = O.ffn_forward(params, sl["obs"])
    dl, dv, st = O.ppo_loss_rows(logits, value, sl["actions"], sl["logits"], sl["logp"], sl["vf_preds"], sl["adv"],
                                 sl["vt"], np.float32(0.2), entropy_coeff=0.0)
    assert stats[0]["kl"] == st["kl"] and stats[0]["policy_loss"] == st["policy_loss"]
    g = O.ffn_backward(params, cache, dl, dv)
    clipped, _ = O.clip_by_global_norm([g[nm] for nm, _ in shapes])
    np.testing.assert_array_equal(glog[0], np.concatenate([c.reshape(-1) for c in clipped]))
    # the mean is over 256 rows: the two 128-row halves' gradients at 1 / 256 each sum to it
    halves = []
    for part in (rows[:128], rows[128:]):
        s2 = {k: v[part] for k, v in batch.items()}
        lg, vl, ch = O.ffn_forward(params, s2["obs"])
        d2, v2, _ = O.ppo_loss_rows(lg, vl, s2["actions"], s2["logits"], s2["logp"], s2["vf_preds"], s2["adv"],
                                    s2["vt"], np.float32(0.2), entropy_coeff=0.0)
        halves.append(O.pack(O.ffn_backward(params, ch, d2 * np.float32(0.5), v2 * np.float32(0.5)), shapes))
    gref = O.pack(g, shapes)
    np.testing.assert_allclose(halves[0] + halves[1], gref, rtol=1e-4, atol=1e-6 * np.abs(gref).max())
    # a 128-row schedule of the same batch is another trajectory
    sh2, pe2 = O.sgd_schedule(np.random.default_rng(3), R, 128, E)
    assert pe2.shape == (E, 4)
    other, _ = O.ppo_update("ffn", params, shapes, O.Adam(n), batch, sh2, pe2, np.float32(0.2),
                            {"entropy_coeff": 0.0}, steps=3)
    assert not np.array_equal(O.pack(other, shapes), O.pack(new, shapes))
