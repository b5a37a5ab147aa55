"""The weight-gradient phase of the fused row-split update after dW1's operands got LDS images of
their own (X, dZ1 beside H1, dZ2) and the two workgroup barriers between the dW2 and the dW1 tiles
went: every image is now rewritten while only a later barrier separates the rewrite from the last
read, so each case runs four epochs of four minibatches = 16 steps -- every image is rewritten 15
times while a neighbouring wave could still be reading it if a lifetime were wrong.  The tile
counts are template constants, so larger shapes run the same code.

Cases: every instance family of the fused dispatch -- the A = 2 kernels in the new form (Local
<2,9>, SharedDecentral <2,5>, SingleNeighbor <2,7>, the LegID env's generic <2,12>, the cup model),
TwoSides (A = 4), Centralized (A = 8, old form: no LDS for the images), and a two-member
UpdateGroup of the Local case (ppo_ffn_group.hip).

Every case asserts (a) theta, m and v against the numpy oracle within test_gpu_parity.py's bar for
parameters after Adam steps, (b) that their SHA-256 digest equals the one recorded from the parent
commit's library (tests/golden/dw_barrier_state.json): no accumulator's order of accumulation and
no sum's operands changed, so the state is the same bit for bit, and (c) that a second run on
fresh contexts gives the same digest -- a wave rewriting an image another wave still reads would
make the result depend on timing.

Recording (the parent commit's libddrl_hip.so copied to ddrl_amd/libddrl_hip_parent.so):

    DDRL_LIB=libddrl_hip_parent.so python -m tests.test_gpu_dw_barrier --record
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from oracle import ddrl_oracle as O
from tests.gpu_harness import (CUP_CONFIG, CUP_ENV, CupOracleRollout, filter_state, init_cup_params, init_params,
                               make_ctx, run_rollout)
from tests.test_gpu_parity import _batch_from_records, _params_close

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dw_barrier_state.json")
EPOCHS, NB, MB, T = 4, 4, 128, 64
STEPS = EPOCHS * NB

# name: env, envs, model config, members.  Rows per policy = T * envs * (agents of the policy) = 4 minibatches.
CASES = {
    "local": ("QuantrupedMultiEnv_Local", 8, None, 1),                     # <2,9>: three dW1 tiles
    "shared_decentral": ("QuantrupedMultiEnv_SharedDecentral", 2, None, 1),   # <2,5>: two dW1 tiles, one shared policy
    "single_neighbor": ("QuantrupedMultiEnv_SingleNeighbor", 8, None, 1),  # <2,7>
    "legid": (CUP_ENV, 2, None, 1),                                        # <2,12>: d = 23, generic k-steps
    "cup": (CUP_ENV, 2, CUP_CONFIG, 1),                                    # <2,5,cup>: coupling table in the partials
    "two_sides": ("QuantrupedMultiEnv_TwoSides", 8, None, 1),             # A = 4
    "centralized": ("QuantrupedMultiEnv_Centralized", 8, None, 1),         # A = 8, old form
    "local_group2": ("QuantrupedMultiEnv_Local", 8, None, 2),              # ppo_ffn_group.hip, two members
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


def _member(name, s):
    """Member s of a case: a context holding the oracle's batch, and what the oracle needs."""
    env, n, config, _ = CASES[name]
    cup = config is CUP_CONFIG
    ctx, cfg, inst = make_ctx(env, n, T, {"num_sgd_iter": EPOCHS, "sgd_minibatch_size": MB, **(config or {})})
    rng = np.random.default_rng(5 + 10 * s)
    params = (init_cup_params if cup else init_params)(ctx, cfg, 7 + s, head_scale=1.0)
    orc, norms, _, _ = run_rollout(ctx, cfg, inst, params, rng, filter_state(cfg.obs_full_dim, rng), T,
                                   **({"orc_cls": CupOracleRollout} if cup else {}))
    shuffles, perms, kls, recs = [], [], [], []
    for p in range(cfg.n_policies):
        lay = ctx.layout[p]
        recs.append(orc.flat_records(p, lay))
        ctx.records_set(p, recs[p])   # the oracle's batch: no rollout rounding inherited
        ctx.adv_norm_set(p, *norms[p])
        R = T * lay["C"]
        assert R == NB * MB, (name, R)
        sh, pe = O.sgd_schedule(np.random.default_rng(100 + p + 50 * s), R, MB, EPOCHS)
        shuffles.append(sh)
        perms.append(pe)
        kls.append(0.2 + 0.1 * p + 0.05 * s)
    return dict(ctx=ctx, cfg=cfg, cup=cup, params=params, recs=recs, norms=norms, shuffles=shuffles, perms=perms, kls=kls)


@functools.lru_cache(maxsize=None)
def run_library(name, rep):
    """[(theta, m, v)] per member and policy after the 16 steps, on fresh contexts (rep: run number)."""
    import torch
    members = [_member(name, s) for s in range(CASES[name][3])]
    dsh = [[torch.from_numpy(x).cuda() for x in mb["shuffles"]] for mb in members]
    dpe = [[torch.from_numpy(x).cuda() for x in mb["perms"]] for mb in members]
    if len(members) == 1:
        mb = members[0]
        mb["ctx"].ppo_update((1 << mb["cfg"].n_policies) - 1, dsh[0], dpe[0], mb["kls"])
        mb["ctx"].synchronize()
        group = None
    else:
        from ddrl_amd.native import UpdateGroup
        group = UpdateGroup([mb["ctx"] for mb in members])
        group.run(dsh, dpe, [mb["kls"] for mb in members])
        group.finish()
    got = []
    for mb in members:
        for p in range(mb["cfg"].n_policies):
            m, v, _, _ = mb["ctx"].adam_get(p)
            got.append((mb["ctx"].params_get(p), np.asarray(m), np.asarray(v)))
    if group is not None:
        group.close()
    for mb in members:
        mb["layout"] = [dict(mb["ctx"].layout[p]) for p in range(mb["cfg"].n_policies)]
        mb.pop("ctx").close()
    return got, members


@functools.lru_cache(maxsize=None)
def run_oracle(name):
    """[(theta, m, v)] of the numpy oracle, in run_library's order, and the learning rate."""
    _, members = run_library(name, 0)
    ref = []
    for mb in members:
        cfg, cup = mb["cfg"], mb["cup"]
        for p in range(cfg.n_policies):
            lay, d, A = mb["layout"][p], cfg.obs_dim[p], cfg.act_dim
            batch = _batch_from_records(mb["recs"][p], lay, d, A, mb["norms"][p])
            if cup:
                batch["leg"] = mb["recs"][p][:, lay["leg"]].astype(np.int64)
            shapes = O.cup_param_shapes(d, A) if cup else O.ffn_param_shapes(d, 2 * A)
            adam = O.Adam(sum(int(np.prod(s)) for _, s in shapes), lr=cfg.lr)
            new, _ = O.ppo_update("cup" if cup else "ffn", mb["params"][p], shapes, adam, batch, mb["shuffles"][p],
                                  mb["perms"][p], np.float32(mb["kls"][p]),
                                  {"entropy_coeff": 0.0, "sgd_minibatch_size": MB})
            ref.append((O.pack(new, shapes), adam.m, adam.v))
    return ref, members[0]["cfg"].lr


def check_oracle(name):
    got, _ = run_library(name, 0)
    ref, lr = run_oracle(name)
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        for what, a, b in zip(("theta", "m", "v"), g, r):
            print(f"{name} #{i} {what}: max |gpu - oracle| {np.abs(a - b).max():.3g}")
            _params_close(a, b, lr, STEPS, f"{name} #{i} {what}")


@pytest.mark.parametrize("name", list(CASES))
def test_state_matches_oracle(name):
    check_oracle(name)


@pytest.mark.parametrize("name", list(CASES))
def test_state_digest_matches_parent(name):
    got, _ = run_library(name, 0)
    with open(GOLDEN) as f:
        golden = json.load(f)["sha256"]
    d = _digest(got)
    print(f"{name}: {d}")
    assert d == golden[name], f"{name}: trained state differs from the parent commit's, bit for bit"


@pytest.mark.parametrize("name", list(CASES))
def test_second_run_gives_the_same_bits(name):
    a, b = _digest(run_library(name, 0)[0]), _digest(run_library(name, 1)[0])
    print(f"{name}: {a} / {b}")
    assert a == b, f"{name}: two runs on fresh contexts differ: the result depends on timing"


def _record():
    import torch
    from ddrl_amd import native as N
    assert torch.cuda.is_available(), "recording needs the GPU"
    out = {"what": "SHA-256 of theta, m, v (fp32 bytes, member by member, policy by policy) after each case of "
                   "tests/test_gpu_dw_barrier.py, from the parent commit's library",
           "recorded_with": "DDRL_LIB=libddrl_hip_parent.so python -m tests.test_gpu_dw_barrier --record",
           "library": os.path.basename(os.environ.get("DDRL_LIB", N.LIB_PATH)),
           "sha256": {name: _digest(run_library(name, 0)[0]) for name in CASES}}
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
