"""The weight-gradient MFMA streams of the fused update (dw_tiles_fm, dw_tiles_fm_head) after their
operand loads moved a row group ahead: every instance family once, two epochs of two minibatches
on seeded records (the second step consumes the weights of the first), at the smallest env count
that gives two minibatches per epoch -- the number of row groups is a template constant, so larger
shapes run the same code.

Every case asserts (a) theta, m and v against the numpy oracle within test_gpu_parity.py's bar for
parameters after Adam steps, and (b) that their SHA-256 digest equals the one recorded from the
parent commit's library (tests/golden/dw_streams_state.json): the change reorders loads and MFMAs
and keeps every accumulator's order of accumulation, so the state is the same bit for bit.

Recording (the parent commit's libddrl_hip.so copied to ddrl_amd/libddrl_hip_parent.so):

    DDRL_LIB=libddrl_hip_parent.so python -m tests.test_gpu_dw_streams --record
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from oracle import ddrl_oracle as O
from tests.gpu_harness import filter_state, init_params, make_ctx, run_rollout
from tests.test_gpu_parity import _batch_from_records, _params_close

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dw_streams_state.json")
EPOCHS = 2

# name: env, envs, T, minibatch.  Rows per policy = T * envs * (agents of the policy) = 2 minibatches.
CASES = {
    "local": ("QuantrupedMultiEnv_Local", 4, 64, 128),                 # <2,9>: three dW1 tiles, head tile on MFMA
    "shared_decentral": ("QuantrupedMultiEnv_SharedDecentral", 1, 64, 128),   # <2,5>: two dW1 tiles
    "two_sides": ("QuantrupedMultiEnv_TwoSides", 4, 64, 128),          # A = 4
    "centralized": ("QuantrupedMultiEnv_Centralized", 4, 64, 128),     # A = 8, compact images
    "local_mb256": ("QuantrupedMultiEnv_Local", 8, 64, 256),           # eight row groups, two row tiles per wave
    "ddp_grad64": ("QuantrupedMultiEnv_SharedDecentral", 1, 64, 128),  # one 64-row gradient export (KSP = 1) + apply
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddrl_amd import build
    build.build()


def _digest(state):
    h = hashlib.sha256()
    for theta, m, v in state:
        for a in (theta, m, v):
            h.update(np.ascontiguousarray(a, np.float32).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def run_case(name):
    """([(theta, m, v)] of the library, the oracle's, lr, steps) per policy of the case."""
    import torch
    env, n, T, mb = CASES[name]
    config = {"num_sgd_iter": EPOCHS, "sgd_minibatch_size": mb}
    ctx, cfg, inst = make_ctx(env, n, T, config)
    rng = np.random.default_rng(5)
    params = init_params(ctx, cfg, 7, head_scale=1.0)
    orc, norms, _, _ = run_rollout(ctx, cfg, inst, params, rng, filter_state(cfg.obs_full_dim, rng), T)
    P = cfg.n_policies
    shuffles, perms, kls = [], [], []
    for p in range(P):
        lay = ctx.layout[p]
        ctx.records_set(p, orc.flat_records(p, lay))   # the oracle's batch: no rollout rounding inherited
        ctx.adv_norm_set(p, *norms[p])
        R = T * lay["C"]
        assert R == 2 * mb, (name, R)
        sh, pe = O.sgd_schedule(np.random.default_rng(100 + p), R, mb, EPOCHS)
        shuffles.append(sh)
        perms.append(pe)
        kls.append(0.2 + 0.1 * p)
    ddp = name == "ddp_grad64"
    steps = 1 if ddp else EPOCHS * 2
    if ddp:
        rows = [np.ascontiguousarray(shuffles[0][:64])]
        g = torch.zeros(ctx.n_params[0], device="cuda")
        ctx.ppo_grad(0, torch.from_numpy(rows[0]).cuda(), 64, kls[0], g)
        ctx.ppo_apply(0, g)
    else:
        ctx.ppo_update((1 << P) - 1, [torch.from_numpy(s).cuda() for s in shuffles],
                       [torch.from_numpy(s).cuda() for s in perms], kls)
    ctx.synchronize()
    got, ref = [], []
    for p in range(P):
        lay = ctx.layout[p]
        d, A = cfg.obs_dim[p], cfg.act_dim
        m, v, _, _ = ctx.adam_get(p)
        got.append((ctx.params_get(p), m, v))
        batch = _batch_from_records(orc.flat_records(p, lay), lay, d, A, norms[p])
        shapes = O.ffn_param_shapes(d, 2 * A)
        adam = O.Adam(sum(int(np.prod(s)) for _, s in shapes), lr=cfg.lr)
        if ddp:
            # the export scales by 1 / sgd_minibatch_size: half of the 64 rows' mean gradient
            sl = {k: a[rows[p]] for k, a in batch.items()}
            logits, value, cache = O.ffn_forward(params[p], sl["obs"])
            dl, dv, _ = O.ppo_loss_rows(logits, value, sl["actions"], sl["logits"], sl["logp"], sl["vf_preds"],
                                        sl["adv"], sl["vt"], np.float32(kls[p]))
            gref = O.pack(O.ffn_backward(params[p], cache, dl, dv), shapes) * np.float32(64 / mb)
            clipped, _ = O.clip_by_global_norm([gref], cfg.grad_clip)
            theta = adam.apply(O.pack(params[p], shapes), clipped[0])
        else:
            new, _ = O.ppo_update("ffn", params[p], shapes, adam, batch, shuffles[p], perms[p], np.float32(kls[p]),
                                  {"entropy_coeff": 0.0, "sgd_minibatch_size": mb})
            theta = O.pack(new, shapes)
        ref.append((theta, adam.m, adam.v))
    lr = cfg.lr
    ctx.close()
    return got, ref, lr, steps


def check_oracle(name):
    got, ref, lr, steps = run_case(name)
    for p, (g, r) in enumerate(zip(got, ref)):
        for what, a, b in zip(("theta", "m", "v"), g, r):
            print(f"{name} p{p} {what}: max |gpu - oracle| {np.abs(a - b).max():.3g}")
            _params_close(a, b, lr, steps, f"{name} p{p} {what}")


@pytest.mark.parametrize("name", list(CASES))
def test_state_matches_oracle(name):
    check_oracle(name)


@pytest.mark.parametrize("name", list(CASES))
def test_state_digest_matches_parent(name):
    got, _, _, _ = run_case(name)
    with open(GOLDEN) as f:
        golden = json.load(f)["sha256"]
    d = _digest(got)
    print(f"{name}: {d}")
    assert d == golden[name], f"{name}: trained state differs from the parent commit's, bit for bit"


def _record():
    import torch
    from ddrl_amd import native as N
    assert torch.cuda.is_available(), "recording needs the GPU"
    out = {"what": "SHA-256 of theta, m, v (fp32 bytes, policy by policy) after each case of "
                   "tests/test_gpu_dw_streams.py, from the parent commit's library",
           "recorded_with": "DDRL_LIB=libddrl_hip_parent.so python -m tests.test_gpu_dw_streams --record",
           "library": os.path.basename(os.environ.get("DDRL_LIB", N.LIB_PATH)),
           "sha256": {name: _digest(run_case(name)[0]) for name in CASES}}
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["sha256"], indent=1))
    for name in CASES:
        check_oracle(name)


if __name__ == "__main__":
    if "--record" in sys.argv:
        _record()
