"""The group update (ddrl_update_group_*, csrc/ppo_ffn_group.hip): M same-shaped contexts updated by
one fused launch, each chain bit-identical to ddrl_ppo_update on a twin context holding the same
state, records and schedule.  The expected values are another run of the project's own kernel, a
chain's arithmetic touches no other chain's data, the exchange admits only this step's tagged
values and the two row halves' sums commute: every comparison is bitwise (a tolerance would hide
exactly what can go wrong here -- a chain reading another chain's outbox or table entry).

Shapes: T = 32 and 256 rows per policy with num_sgd_iter = 2, i.e. 2 minibatches x 2 epochs = 4
steps, so both values of the quads' tag bit and both outbox parities occur.  Every member has its
own seed for weights, records, shuffle and perm, and its own KL coefficients."""
import os

import numpy as np
import pytest

from tests.gpu_harness import CUP_CONFIG, CUP_ENV, GNN_ENV, init_policy_params, make_ctx

pytestmark = pytest.mark.gpu
LOCAL, C4 = "QuantrupedMultiEnv_Local", "QuantrupedMultiEnv_SharedDecentral"
T, EPOCHS, STEPS = 32, 2, 4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ctx(env, n, config=None, **envvars):
    old = {k: os.environ.get(k) for k in envvars}
    os.environ.update({k: str(v) for k, v in envvars.items()})
    try:
        return make_ctx(env, n, T, {"num_sgd_iter": EPOCHS, **(config or {})})
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _schedule(ctx, seed):
    """(shuffles, perms, kl) of one update of a context, seeded."""
    import torch
    rng = np.random.default_rng(seed)
    sh, pe = [], []
    for p in range(ctx.cfg.n_policies):
        R = T * ctx.layout[p]["C"]
        assert R == 256
        sh.append(torch.from_numpy(rng.permutation(R).astype(np.int32)).cuda())
        pe.append(torch.from_numpy(np.stack([rng.permutation(R // 128) for _ in range(EPOCHS)]).astype(np.int32)).cuda())
    return sh, pe, [float(k) for k in rng.uniform(0.1, 0.5, ctx.cfg.n_policies)]


def _member(env, n, seed, config=None, **envvars):
    """A context with seeded weights, Adam state away from the start, and a seeded fragment."""
    from ddrl_amd.synthetic import SyntheticRollout
    ctx, cfg, _ = _ctx(env, n, config, **envvars)
    init_policy_params(ctx, cfg, 100 + seed, bool(cfg.leg_coupling))
    rng = np.random.default_rng(200 + seed)
    for p in range(cfg.n_policies):
        k = ctx.n_params[p]
        ctx.adam_set(p, rng.normal(size=k).astype(np.float32) * 1e-3, rng.uniform(1e-7, 1e-5, k).astype(np.float32),
                     0.9 ** 3, 0.999 ** 3)
    syn = SyntheticRollout(n, T, cfg.obs_full_dim, cfg.n_agents, cfg.act_dim, "cuda:0", seed=300 + seed)
    ctx.observe(syn.obs[0])
    ctx.rollout_fragment(syn.obs, syn.eps, syn.fw, syn.cfrc, syn.dones_for_fragment(), syn.actions)
    ctx.gae()
    ctx.synchronize()
    return ctx


def _twin(src, env, n, config=None):
    """A second context holding src's weights, Adam state, records and advantage constants."""
    ctx, cfg, _ = _ctx(env, n, config)
    for p in range(cfg.n_policies):
        ctx.params_set(p, src.params_get(p))
        ctx.adam_set(p, *src.adam_get(p))
        ctx.records_set(p, src.records_get(p))
        ctx.adv_norm_set(p, *[float(x) for x in src.adv_norm_get(p)])
    ctx.synchronize()
    return ctx


def _state(ctx, steps=STEPS):
    """theta, m, v, beta powers and every ppo_stats row of every policy."""
    out = []
    for p in range(ctx.cfg.n_policies):
        m, v, b1, b2 = ctx.adam_get(p)
        out += [ctx.params_get(p), m, v, np.array([b1, b2], np.float32), ctx.ppo_stats(p, steps)]
    return out


def _hw_state(ctx):
    return [x for i, x in enumerate(_state(ctx, 0)) if i % 5 != 4]


def _assert_same(got, ref, what):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: item {i} (policy {i // 5}, "
                                                    f"{('theta', 'm', 'v', 'beta powers', 'stats')[i % 5]})")


def _solo(ctx, sched, max_steps=-1):
    sh, pe, kl = sched
    ctx.ppo_update((1 << ctx.cfg.n_policies) - 1, sh, pe, kl, max_steps=max_steps)
    ctx.synchronize()


def _group_vs_twins(env, n, M, config=None, cap=0, rounds=1):
    """M members updated by one group `rounds` times, against their twins' solo updates."""
    from ddrl_amd.native import UpdateGroup
    members = [_member(env, n, s, config) for s in range(M)]
    twins = [_twin(c, env, n, config) for c in members]
    group = UpdateGroup(members, cap)
    for r in range(rounds):
        scheds = [_schedule(c, 1000 * r + 10 + s) for s, c in enumerate(members)]
        assert len({tuple(s[2]) for s in scheds}) == M          # every member its own KL coefficients
        group.run([s[0] for s in scheds], [s[1] for s in scheds], [s[2] for s in scheds])
        group.finish()
        for s, (c, t) in enumerate(zip(members, twins)):
            _solo(t, scheds[s])
            _assert_same(_state(c), _state(t), f"{env} M={M} cap={cap} round {r} member {s}")
    # the members' updates differ from each other (a chain that ran another's table entry would show)
    if M > 1:
        assert not np.array_equal(members[0].params_get(0), members[1].params_get(0))
    return group, members, twins


def _close(group, *ctx_lists):
    group.close()
    for cs in ctx_lists:
        for c in cs:
            c.close()


@pytest.mark.parametrize("M", [1, 2, 3])
def test_local_members_match_solo_twins(M):
    """M = 2 fills all eight slots of group row 0; M = 3 crosses into row 1 and leaves its slots 4-7 empty."""
    _close(*_group_vs_twins(LOCAL, 8, M))


def test_shared_policy_nine_members():
    """C4: one chain per member; chain 8 sits alone in group row 1."""
    _close(*_group_vs_twins(C4, 2, 9))


@pytest.mark.parametrize("env,n,config", [
    ("QuantrupedMultiEnv_Centralized", 8, None),       # A = 8: the instance with all 512 registers, compact images
    ("QuantrupedMultiEnv_TwoSides", 8, None),          # A = 4
    (CUP_ENV, 2, CUP_CONFIG),                          # the "cup" model: coupling table in the policy branch
    (CUP_ENV, 2, None),                                # LegID env, fcnet: d = 23, the generic KS1 = 12 instance
], ids=["centralized", "twosides", "cup", "legid"])
def test_member_pair_of_every_kernel_family(env, n, config):
    group, members, twins = _group_vs_twins(env, n, 2, config)
    if env == CUP_ENV and config is None:
        assert members[0].cfg.obs_dim[0] == 23
    _close(group, members, twins)


def test_split_launches_give_the_same_bits():
    """Local M = 3 with at most 8 chains per launch: two launches (members 0-1, member 2)."""
    from ddrl_amd.native import update_group_plan
    lom, _ = update_group_plan(3, 4, 8)
    assert list(lom) == [0, 0, 1]
    one = _group_vs_twins(LOCAL, 8, 3)
    two = _group_vs_twins(LOCAL, 8, 3, cap=8)
    for s, (a, b) in enumerate(zip(one[1], two[1])):
        _assert_same(_state(a), _state(b), f"one launch against two, member {s}")
    assert len(two[0].placement()) == 32 + 24 + 4
    _close(*one)
    _close(*two)


def test_repeated_runs_on_one_group():
    """Two run / finish rounds with new schedules: the launch epoch, the outbox clear and the reuse of
    the pinned table."""
    _close(*_group_vs_twins(LOCAL, 8, 2, rounds=2))


def test_failed_run_restores_every_member():
    from ddrl_amd.native import DdrlError, UpdateGroup
    members = [_member(LOCAL, 8, 0), _member(LOCAL, 8, 1, DDRL_TEST_FAIL_STEP=1), _member(LOCAL, 8, 2)]
    before = [_hw_state(c) for c in members]
    group = UpdateGroup(members)
    scheds = [_schedule(c, 10 + s) for s, c in enumerate(members)]
    group.run([s[0] for s in scheds], [s[1] for s in scheds], [s[2] for s in scheds])
    with pytest.raises(DdrlError, match="of every member are as before the call"):
        group.finish()
    for c, b in zip(members, before):
        for x, y in zip(_hw_state(c), b):
            np.testing.assert_array_equal(x, y)
    # a later, unrelated check on a member restores nothing: state written now survives it
    marked = members[0].params_get(0) + np.float32(1.0)
    members[0].params_set(0, marked)
    for c in members:
        c.synchronize()
    np.testing.assert_array_equal(members[0].params_get(0), marked)
    _close(group, members)


def test_placement_one_xcd_per_chain():
    from ddrl_amd.native import update_group_grid, update_group_plan
    group, members, twins = _group_vs_twins(LOCAL, 8, 3)
    xcc = group.placement()
    assert xcc.size == update_group_grid(12) == 32 + 24 + 4
    _, first = update_group_plan(3, 4, 64)
    for b in first.ravel():
        ids = {int(xcc[b + 8 * j]) for j in range(4)}
        assert len(ids) == 1 and 0 <= ids.pop() < 8, f"chain at block {b}: {xcc[b:b + 25:8]}"
    _close(group, members, twins)


# ---- refusals ----

def _refused(contexts, match, cap=0):
    from ddrl_amd.native import DdrlError, UpdateGroup
    with pytest.raises(DdrlError, match=match):
        UpdateGroup(contexts, cap)


def test_create_refusals():
    import torch
    a, cfg, _ = _ctx(LOCAL, 8)
    b, _, _ = _ctx(LOCAL, 8)
    _refused([], "at least one member")
    _refused([a, a], "member 1 repeats member 0")
    other = torch.cuda.Stream()
    s, _, _ = make_ctx(LOCAL, 8, T, {"num_sgd_iter": EPOCHS}, stream=other.cuda_stream)
    _refused([a, s], "member 1 is on another stream")
    _refused([a, b], "cannot hold a member's 4", cap=3)
    for config, why in (({"num_sgd_iter": 3}, "num_sgd_iter"), ({"lr": 1e-4}, "lr"), ({"clip_param": 0.3}, "clip_param"),
                        ({"entropy_coeff": 0.01}, "entropy_coeff")):
        d, _, _ = _ctx(LOCAL, 8, config)
        _refused([a, d], f"member 1 differs from member 0 in {why}")
        d.close()
    d, _, _ = _ctx(LOCAL, 16)
    _refused([a, d], "member 1 differs from member 0 in frag_len x n_envs")
    d.close()
    d, _, _ = _ctx(C4, 8)
    _refused([a, d], "member 1 differs from member 0 in n_policies")
    d.close()
    d, _, _ = _ctx("QuantrupedMultiEnv_FullyDecentral", 8)
    _refused([a, d], "member 1 differs from member 0 in obs_dim")
    d.close()
    d, _, _ = _ctx(CUP_ENV, 2)
    e, _, _ = _ctx(CUP_ENV, 2, CUP_CONFIG)
    _refused([d, e], "member 1 differs from member 0 in leg_coupling")
    d.close()
    e.close()
    d, _, _ = _ctx(GNN_ENV, 8)
    _refused([d], "member 0 is a GraphNet context")
    d.close()
    d, _, _ = _ctx(LOCAL, 16, {"sgd_minibatch_size": 256})
    _refused([d], "member 0 has sgd_minibatch_size 256")
    d.close()
    d, _, _ = _ctx(LOCAL, 8, DDRL_UPDATE_SPLIT=1)
    _refused([a, d], "member 1 was created under DDRL_UPDATE_SPLIT=1")
    d.close()
    d, _, _ = _ctx(LOCAL, 8, DDRL_XCHG="atomic")
    _refused([a, d], "member 1 is on the atomic exchange protocol")
    d.close()
    for c in (a, b, s):
        c.close()


def test_peer_member_is_refused():
    a, _, _ = _ctx(C4, 2)
    b, _, _ = _ctx(C4, 2)
    gx, _ = a.peer_alloc()
    a.peer_attach(gx, 0)
    _refused([b, a], "member 1 is attached to a peer")
    a.close()
    b.close()


def test_group_use_after_close_and_unfinished_run():
    from ddrl_amd.native import DdrlError, UpdateGroup
    members = [_member(C4, 2, 0)]
    group = UpdateGroup(members)
    sh, pe, kl = _schedule(members[0], 1)
    group.run([sh], [pe], [kl])
    with pytest.raises(DdrlError, match="previous run has not been finished"):
        group.run([sh], [pe], [kl])
    group.finish()
    with pytest.raises(DdrlError, match="null shuffle/perm"):
        group.run([[None]], [pe], [kl])
    group.close()
    for call in (lambda: group.run([sh], [pe], [kl]), group.finish, group.placement):
        with pytest.raises(DdrlError, match="used after close"):
            call()
    members[0].close()
