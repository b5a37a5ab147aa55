"""Evaluation members (ddrl_eval_members_*; eval_members.hip): M parameter sets side by side on
one context, n envs each, against M plain contexts of n envs holding the same state.  The contract
is bit equality with kernels that already exist (k_eval_act, the env-side filter push, the device
env plane), so every comparison is assert_array_equal: there is no tolerance to choose.

Reference: evaluation/evaluate_trained_policies_pd.py:84-127 and
evaluate_trained_policies_tvel_range_pd.py:80-102 (one restored agent per sweep cell)."""
import numpy as np
import pytest

from ddrl_amd import native as N
from tests.gpu_harness import CUP_CONFIG, CUP_ENV, dev, init_policy_params, make_ctx

pytestmark = pytest.mark.gpu
LOCAL = "QuantrupedMultiEnv_Local"
LIMIT = 20
TVS = [0.5, 1.0, 2.0]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def assert_bits(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def _is_cup(config):
    return bool(config and (config.get("model") or {}).get("custom_model") == "cup")


def _filt(D, rng):
    return 100.0 + float(rng.integers(0, 50)), rng.normal(size=D) * 0.1, np.abs(rng.normal(size=D)) * 99 + 1


def _pfilt(cfg, rng):
    return [(500.0 + float(rng.integers(0, 50)), rng.normal(size=cfg.obs_dim[p]) * 0.2,
             np.abs(rng.normal(size=cfg.obs_dim[p])) * 499 + 5) for p in range(cfg.n_policies)]


def _set_state(ctx, cfg, seed, cup, rng):
    """Seeded parameters, env-side filter and per-policy filters into ctx; returns what was set."""
    init_policy_params(ctx, cfg, seed, cup)
    filt = _filt(cfg.obs_full_dim, rng)
    ctx.filter_set(*filt)
    pf = _pfilt(cfg, rng) if cfg.policy_filter else None
    for p in range(cfg.n_policies if pf else 0):
        ctx.policy_filter_set(p, *pf[p])
    return filt, pf


def _own_state(ctx, cfg):
    out = {"params": [ctx.params_get(p) for p in range(cfg.n_policies)], "filter": ctx.filter_get(),
           "delta": ctx.filter_delta_get()}
    if cfg.policy_filter:
        out["pf"] = [ctx.policy_filter_get(p) for p in range(cfg.n_policies)]
    return out


def _assert_state_equal(a, b):
    for x, y in zip(a["params"], b["params"]):
        assert_bits(x, y, "the context's own parameters")
    for key in ("filter", "delta"):
        for x, y in zip(a[key], b[key]):
            assert_bits(np.asarray(x, np.float64), np.asarray(y, np.float64), f"the context's own {key}")
    for fa, fb in zip(a.get("pf", []), b.get("pf", [])):
        for x, y in zip(fa, fb):
            assert_bits(np.asarray(x, np.float64), np.asarray(y, np.float64), "the context's own per-policy filter")


def _members(env, M, n, config, filter_update, E=1):
    """A member context of M * n envs with every member loaded from a plain context of n envs, and
    those plain contexts.  The member context's own state is set to something else afterwards."""
    cup = _is_cup(config)
    mctx, mcfg, _ = make_ctx(env, M * n, 1, config)
    rng = np.random.default_rng(77)
    mctx.eval_begin(E, filter_update=filter_update)
    mctx.eval_members_begin(M)
    plain = []
    for m in range(M):
        pctx, pcfg, _ = make_ctx(env, n, 1, config)
        filt, pf = _set_state(pctx, pcfg, 5 + m, cup, rng)
        for p in range(pcfg.n_policies):
            mctx.params_set(p, pctx.params_get(p))
            if pf:
                mctx.policy_filter_set(p, *pf[p])
        mctx.filter_set(*filt)
        mctx.eval_member_load(m)
        pctx.eval_begin(1, filter_update=filter_update)
        plain.append(pctx)
    _set_state(mctx, mcfg, 99, cup, rng)   # the context's own state: no member's
    mctx.synchronize()
    return mctx, mcfg, plain


def _logit_bufs(ctx, cfg):
    import torch
    return [torch.full((ctx.layout[p]["C"], 2 * cfg.act_dim), float("nan"), dtype=torch.float32, device="cuda")
            for p in range(cfg.n_policies)]


def _close(*ctxs):
    for c in ctxs:
        c.close()


MEMBER_CASES = [
    # one full workgroup plus a ragged tile per member, per-policy filters
    pytest.param(LOCAL, 3, 70, {"observation_filter": "MeanStdFilter"}, id="local_pfilter_3x70"),
    pytest.param("QuantrupedMultiEnv_SharedDecentral", 3, 5, None, id="shared_3x5"),        # k = 4: 20 rows
    pytest.param(CUP_ENV, 2, 19, CUP_CONFIG, id="cup_2x19"),                                # coupling, constants
    pytest.param("QuantrupedMultiEnv_Centralized", 2, 70, None, id="centralized_2x70"),     # A = 8
    pytest.param("QuantrupedMultiEnv_FullyDecentral", 2, 37, {"env_config": {"target_velocity": [1.0]}},
                 id="tvel_2x37"),                                                           # D = 44
]


@pytest.mark.parametrize("env,M,n,config", MEMBER_CASES)
def test_member_act_parity(env, M, n, config):
    """One member-mode eval_act against M plain contexts of n envs with the same state, each fed its
    slice of the same obs / eps: actions and logits bit for bit, with noise and without; the member
    context's own parameters and filters (which are no member's) read back unchanged."""
    import torch
    mctx, cfg, plain = _members(env, M, n, config, filter_update=False)
    assert cfg.obs_full_dim == (44 if "target_velocity" in str(config) else 43)
    own = _own_state(mctx, cfg)
    rng = np.random.default_rng(31)
    obs = (rng.normal(size=(M * n, cfg.obs_full_dim)) * 2 + 0.5).astype(np.float32)
    eps = rng.normal(size=(M * n, cfg.n_agents, cfg.act_dim)).astype(np.float32)
    o_all = dev(obs)
    for noise in (True, False):
        e_all = dev(eps) if noise else None
        act_m = torch.full((M * n, 8), float("nan"), dtype=torch.float32, device="cuda")
        lg_m = _logit_bufs(mctx, cfg)
        mctx.eval_act(o_all, e_all, act_m, lg_m)
        mctx.synchronize()
        got_a = act_m.cpu().numpy()
        assert np.isfinite(got_a).all()
        for m, pctx in enumerate(plain):
            sl = slice(m * n, (m + 1) * n)
            act_p = torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda")
            lg_p = _logit_bufs(pctx, cfg)
            pctx.eval_act(dev(obs[sl]), dev(eps[sl]) if noise else None, act_p, lg_p)
            pctx.synchronize()
            assert_bits(got_a[sl], act_p.cpu().numpy(), f"member {m} actions (noise={noise})")
            for p in range(cfg.n_policies):
                C_p = pctx.layout[p]["C"]
                assert_bits(lg_m[p].cpu().numpy()[m * C_p:(m + 1) * C_p], lg_p[p].cpu().numpy(),
                            f"member {m} policy {p} logits (noise={noise})")
        if M > 1:   # the members really differ
            assert not np.array_equal(got_a[:n], got_a[n:2 * n])
    _assert_state_equal(_own_state(mctx, cfg), own)
    for m, pctx in enumerate(plain):   # a frozen filter does not move
        for x, y in zip(mctx.eval_member_filter_get(m), pctx.filter_get()):
            assert_bits(np.asarray(x, np.float64), np.asarray(y, np.float64), f"member {m} frozen filter")
    mctx.eval_end()
    _close(mctx, *plain)


FILTER_CASES = [
    pytest.param(LOCAL, 2, 260, None, id="local_2x260"),   # two chunks per member, the second ragged
    # D = 44: the merge kernel's 44th column is live; the second chunk is a single row; member 1 is
    # neither the first nor the last z, where a count added once per launch or to a neighbour would show
    pytest.param("QuantrupedMultiEnv_FullyDecentral", 3, 257, {"env_config": {"target_velocity": [1.0]}},
                 id="tvel_3x257"),
]


@pytest.mark.parametrize("env,M,n,config", FILTER_CASES)
def test_member_filter_continues(env, M, n, config):
    """filter_update = 1 over three steps, two chunks per member (the second ragged): the actions of
    every step and the final running stat of every member are those of its plain context, and the
    count of every member (advanced by the act kernel behind the merge) is exactly 3 n further."""
    import torch
    mctx, cfg, plain = _members(env, M, n, config, filter_update=True)
    assert cfg.obs_full_dim == (44 if config else 43)
    own = _own_state(mctx, cfg)
    rng = np.random.default_rng(32)
    act_m = torch.full((M * n, 8), float("nan"), dtype=torch.float32, device="cuda")
    act_p = torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda")
    before = [pctx.filter_get() for pctx in plain]
    for t in range(3):
        obs = (rng.normal(size=(M * n, cfg.obs_full_dim)) * (1.0 + t) + 0.5 * t).astype(np.float32)
        mctx.eval_act(dev(obs), None, act_m)
        mctx.synchronize()
        got = act_m.cpu().numpy()
        for m, pctx in enumerate(plain):
            sl = slice(m * n, (m + 1) * n)
            pctx.eval_act(dev(obs[sl]), None, act_p)
            pctx.synchronize()
            assert_bits(got[sl], act_p.cpu().numpy(), f"step {t} member {m} actions")
    for m, pctx in enumerate(plain):
        got, want = mctx.eval_member_filter_get(m), pctx.filter_get()
        assert got[0] == want[0] == before[m][0] + 3 * n
        assert_bits(got[1], want[1], f"member {m} filter mean")
        assert_bits(got[2], want[2], f"member {m} filter M2")
        assert not np.array_equal(want[1], before[m][1])
    _assert_state_equal(_own_state(mctx, cfg), own)
    mctx.eval_end()
    _close(mctx, *plain)


def test_member_loop_equals_plain_contexts():
    """ddrl_eval_devenv in member mode against a hand-written loop over a second device env of the
    same seed: member m's actions from plain context m on its slice of the observations, the
    accounting by a plain context of all M * n envs."""
    import torch
    M, n, E, poll = 3, 8, 2, 5
    Nn, max_steps = M * n, E * LIMIT
    mctx, cfg, plain = _members(LOCAL, M, n, None, filter_update=True, E=E)
    actx, _, _ = make_ctx(LOCAL, Nn, 1)
    rng = np.random.default_rng(6)
    eps = dev(rng.normal(size=(max_steps, Nn, cfg.n_agents, cfg.act_dim)).astype(np.float32))
    ea, eb = N.DevEnv(mctx, seed=21), N.DevEnv(actx, seed=21)
    for env in (ea, eb):
        env.set_time_limit(LIMIT)
    steps_a = mctx.eval_devenv(ea, eps, max_steps, max_steps, poll_every=poll)

    actx.eval_begin(E, filter_update=False)
    actions = torch.zeros((Nn, 8), dtype=torch.float32, device="cuda")
    eb.reset_episodes()
    steps_b = 0
    while steps_b < max_steps:
        for m, pctx in enumerate(plain):
            sl = slice(m * n, (m + 1) * n)
            pctx.eval_act(eb.obs[sl], eps[steps_b][sl], actions[sl])
            pctx.synchronize()
        eb.step(actions)
        actx.eval_step(eb.fw, eb.cfrc, actions, eb.kin, eb.done)
        actx.synchronize()
        steps_b += 1
        if steps_b % poll == 0 and actx.eval_progress()[1] == Nn:
            break
    assert steps_a == steps_b and 1 < steps_a <= max_steps
    ta, tb = mctx.eval_results(), actx.eval_results()
    assert_bits(ta, tb, "result table")
    assert not np.isnan(ta[:, :, :5]).any()
    assert mctx.eval_progress() == actx.eval_progress() == (Nn * E, Nn)
    for m, pctx in enumerate(plain):
        for x, y in zip(mctx.eval_member_filter_get(m), pctx.filter_get()):
            assert_bits(np.asarray(x, np.float64), np.asarray(y, np.float64), f"member {m} env-side filter")
    assert_bits(ea.state(), eb.state(), "env state")
    mctx.eval_end()
    actx.eval_end()
    for env in (ea, eb):
        env.close()
    _close(mctx, actx, *plain)


def _scripted_actions(n, t):
    return np.random.default_rng(1000 + t).uniform(-1.0, 1.0, size=(n, 8)).astype(np.float32)


def test_per_env_target_velocities():
    """A table of distinct velocities on a D = 44 env: every reset and every episode restart inside
    the step kernel takes the env's own value; None goes back to drawing from the list, and the env
    is then a fresh env of the same seed and list again."""
    n = 70
    config = {"env_config": {"target_velocity": TVS}}
    ctx, cfg, _ = make_ctx(LOCAL, n, 1, config)
    assert cfg.obs_full_dim == 44
    denv = N.DevEnv(ctx, seed=43, target_velocity=TVS)
    denv.set_time_limit(LIMIT)
    table = (0.25 + 0.03125 * np.arange(n)).astype(np.float32)   # distinct, exact in fp32
    denv.set_env_target_velocities(table)

    def check(what):
        ctx.synchronize()
        assert_bits(denv.target_velocities, table, f"{what}: target velocities")
        assert_bits(denv.obs.cpu().numpy()[:, 43], table, f"{what}: observation column")

    denv.reset()
    check("reset")
    denv.reset_episodes()
    check("reset_episodes")
    ends = np.zeros(n, np.int64)
    for t in range(2 * LIMIT + 2):
        denv.step(dev(_scripted_actions(n, t)))
        ctx.synchronize()
        ends += denv.done.cpu().numpy()
        if t % 7 == 0:
            check(f"step {t}")
    check("after the episodes")
    assert (ends >= 2).all()          # every env restarted inside the step kernel, more than once
    denv.reset_state()                # keeps the velocities
    assert_bits(denv.target_velocities, table, "reset_state")

    denv.set_env_target_velocities(None)
    fresh = N.DevEnv(ctx, seed=43, target_velocity=TVS)
    fresh.set_time_limit(LIMIT)
    for what, call in (("reset", "reset"), ("reset_episodes", "reset_episodes")):
        getattr(denv, call)()
        getattr(fresh, call)()
        ctx.synchronize()
        assert_bits(denv.state(), fresh.state(), f"list drawing restored: {what} state")
        assert_bits(denv.obs.cpu().numpy(), fresh.obs.cpu().numpy(), f"list drawing restored: {what} obs")
        assert set(np.unique(denv.target_velocities)) <= set(np.float32(TVS))
    assert len(set(np.unique(denv.target_velocities))) > 1
    for t in range(LIMIT + 1):        # and the restarts inside the step kernel draw from the list again
        a = dev(_scripted_actions(n, t))
        denv.step(a)
        fresh.step(a)
    ctx.synchronize()
    assert_bits(denv.state(), fresh.state(), "list drawing restored: stepped state")

    for bad, msg in ((float("nan"), "finite"), (float("inf"), "finite"), (0.0, "> 0"), (-1.0, "> 0")):
        t2 = table.copy()
        t2[n // 2] = bad
        with pytest.raises(N.DdrlError, match=msg):
            denv.set_env_target_velocities(t2)
    with pytest.raises(N.DdrlError, match="n_envs floats"):
        denv.set_env_target_velocities(table[:-1])
    with pytest.raises(N.DdrlError, match="null device env"):
        N._ck(N.load().ddrl_devenv_set_env_target_velocities(None, None, 0))
    ctx43, _, _ = make_ctx(LOCAL, 5, 1)
    flat = N.DevEnv(ctx43, seed=1)
    flat.set_env_target_velocities([0.0, -1.0, 1.0, 2.0, 3.0])   # D = 43: any finite value
    with pytest.raises(N.DdrlError, match="finite"):
        flat.set_env_target_velocities([0.0, float("nan"), 1.0, 2.0, 3.0])
    for env in (denv, fresh, flat):
        env.close()
    _close(ctx, ctx43)


def test_member_messages_and_leaving_the_mode():
    import torch
    n = 12
    ctx, cfg, _ = make_ctx(LOCAL, n, 1)
    twin, _, _ = make_ctx(LOCAL, n, 1)
    rng = np.random.default_rng(3)
    for c in (ctx, twin):
        _set_state(c, cfg, 5, False, np.random.default_rng(4))
    obs = dev((rng.normal(size=(n, 43)) * 2).astype(np.float32))
    actions = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(N.DdrlError, match="ddrl_eval_begin first"):
        ctx.eval_members_begin(2)
    ctx.eval_begin(1)
    with pytest.raises(N.DdrlError, match="ddrl_eval_members_begin first"):
        ctx.eval_member_load(0)
    with pytest.raises(N.DdrlError, match="must divide n_envs"):
        ctx.eval_members_begin(5)
    for bad in (0, -3):
        with pytest.raises(N.DdrlError, match="n_members must be >= 1"):
            ctx.eval_members_begin(bad)
    ctx.eval_members_begin(3)
    for bad in (-1, 3):
        with pytest.raises(N.DdrlError, match="out of range"):
            ctx.eval_member_load(bad)
        with pytest.raises(N.DdrlError, match="out of range"):
            ctx.eval_member_filter_get(bad)
    ctx.eval_member_load(0)
    ctx.eval_member_load(2)
    with pytest.raises(N.DdrlError, match="member 1 has not been loaded"):
        ctx.eval_act(obs, None, actions)
    with pytest.raises(N.DdrlError, match="member mode"):
        ctx.eval_sens_begin([np.full(cfg.obs_dim[p], 0.1) for p in range(cfg.n_policies)])
    henv = N.HostEnv(n, 43, n_threads=1, seed=1)
    with pytest.raises(N.DdrlError, match="member mode"):
        ctx.eval_hostenv(henv, max_steps=5)
    henv.close()
    with pytest.raises(N.DdrlError, match="null context"):
        N._ck(N.load().ddrl_eval_members_begin(None, 1))
    ctx.eval_member_load(1)
    ctx.eval_act(obs, None, actions)
    ctx.synchronize()
    # eval_end leaves the mode: the plain path again, bit-equal to a context that never entered it
    ctx.eval_end()
    with pytest.raises(N.DdrlError, match="ddrl_eval_begin first"):
        ctx.eval_member_load(0)
    got = torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda")
    want = torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda")
    for c, out in ((ctx, got), (twin, want)):
        c.eval_begin(1, filter_update=True)
        c.eval_act(obs, None, out)
        c.synchronize()
    with pytest.raises(N.DdrlError, match="ddrl_eval_members_begin first"):
        ctx.eval_member_load(0)      # the next eval_begin ended the mode too
    assert_bits(got.cpu().numpy(), want.cpu().numpy(), "plain eval_act after the member mode")
    for x, y in zip(ctx.filter_get(), twin.filter_get()):
        assert_bits(np.asarray(x, np.float64), np.asarray(y, np.float64), "plain filter after the member mode")
    # GraphNet contexts stay refused
    from tests.gpu_harness import GNN_ENV
    gctx, _, _ = make_ctx(GNN_ENV, 4, 1)
    with pytest.raises(N.DdrlError, match="fcnet models only"):
        gctx.eval_begin(1)
    with pytest.raises(N.DdrlError, match="ddrl_eval_begin first"):
        gctx.eval_members_begin(2)
    for c in (ctx, twin):
        c.eval_end()
    _close(ctx, twin, gctx)
