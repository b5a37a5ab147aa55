"""The group finish (ddrl_finish_group_*, csrc/finish_group.hip): GAE and the episode accounting of
M same-shaped contexts as one chain of launches, every member bit-identical to ddrl_gae +
ddrl_episodes_collect on a twin context brought to the same state by the same seeded synthetic
rollout and scripted done flags.  The group kernels include the plain kernels' texts and run the
same fp64 additions in the same order, so every comparison is assert_array_equal: a tolerance would
hide what can go wrong here -- a member reading another member's table entry, base or totals.

Shapes: the kernels' time chunk is 16, so T in {1, 17, 33} is a single step, a ragged second chunk
and a ragged third; n in {3, 65, 130} is below a wave, a ragged second wave and a ragged third.
SharedDecentral (k = 4) at n = 20 / 65 has C = 80 / 260 chains: two GAE waves, and five waves with
a ragged second group of four in the finalize."""
import ctypes as C

import numpy as np
import pytest

from ddrl_amd import native as N
from tests.gpu_harness import GNN_ENV, dev, init_gnn_params, init_params, make_ctx, synthetic_inputs

pytestmark = pytest.mark.gpu
LOCAL, C4 = "QuantrupedMultiEnv_Local", "QuantrupedMultiEnv_SharedDecentral"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---- members and twins --------------------------------------------------------------------------
def _ctx(env, n, T, seed, config=None, cfg_set=None):
    ctx, cfg, _ = make_ctx(env, n, T, config, cfg_set=cfg_set)
    if cfg.model_kind == N.MODEL_GNN:
        init_gnn_params(ctx, 100 + seed)
    else:
        init_params(ctx, cfg, 100 + seed)
    return ctx


def _pairs(env, n, T, M, config=None):
    """M (member, twin) pairs; member m and its twin hold the same seeded weights."""
    return [(_ctx(env, n, T, m, config), _ctx(env, n, T, m, config)) for m in range(M)]


def _fragment(ctx, seed, done):
    """One fragment of seeded synthetic inputs with the scripted done flags, up to the bootstrap."""
    import torch
    cfg = ctx.cfg
    T, n = done.shape
    obs, eps, fw, cfrc, _ = synthetic_inputs(np.random.default_rng(seed), cfg, T)
    actions = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    for t in range(T):
        ctx.observe(dev(obs[t]))
        ctx.act(t, dev(eps[t]), actions)
        ctx.reward(t, dev(fw[t]), dev(cfrc[t]), actions, dev(done[t]))
    ctx.observe(dev(obs[T]))
    ctx.bootstrap()
    ctx.synchronize()


def _fragments(pairs, dones, seed):
    for m, (c, t) in enumerate(pairs):
        _fragment(c, 1000 * seed + m, dones[m])
        _fragment(t, 1000 * seed + m, dones[m])


def _plain(ctx):
    ctx.gae()
    return ctx.episodes_collect()


def _assert_same_member(c, t, rows, want, what):
    assert rows.dtype == np.float64 and rows.shape == want.shape, (what, rows.shape, want.shape)
    np.testing.assert_array_equal(rows, want, err_msg=f"{what}: episode rows")
    for p in range(c.cfg.n_policies):
        lay = c.layout[p]
        got_rec, want_rec = c.records_get(p), t.records_get(p)
        for col in ("adv", "vt"):
            np.testing.assert_array_equal(got_rec[:, lay[col]], want_rec[:, lay[col]], err_msg=f"{what}: policy {p} {col}")
        np.testing.assert_array_equal(got_rec, want_rec, err_msg=f"{what}: policy {p} records")
        np.testing.assert_array_equal(c.adv_norm_get(p), t.adv_norm_get(p), err_msg=f"{what}: policy {p} adv_norm")
        np.testing.assert_array_equal(c.adv_sums_get(p), t.adv_sums_get(p), err_msg=f"{what}: policy {p} adv_sums")
    np.testing.assert_array_equal(c.episodes_inflight(), t.episodes_inflight(), err_msg=f"{what}: in-flight state")


def _run_and_compare(group, pairs, what):
    got = group.run()
    assert len(got) == len(pairs)
    for m, ((c, t), rows) in enumerate(zip(pairs, got)):
        _assert_same_member(c, t, rows, _plain(t), f"{what} member {m}")
    return got


def _close(group, pairs):
    group.close()
    for c, t in pairs:
        c.close()
        t.close()


def _random_dones(rng, M, T, n, p=0.1):
    return [(rng.random(size=(T, n)) < p).astype(np.uint8) for _ in range(M)]


# ---- equality with the plain path ---------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 17, 33])
@pytest.mark.parametrize("n", [3, 65, 130])
def test_local_three_members_every_shape(n, T):
    rng = np.random.default_rng(100 * n + T)
    pairs = _pairs(LOCAL, n, T, 3)
    group = N.FinishGroup([c for c, _ in pairs])
    for f in range(2):   # the second fragment starts from in-flight state
        dones = _random_dones(rng, 3, T, n)
        _fragments(pairs, dones, 10 * n + f)
        got = _run_and_compare(group, pairs, f"Local n={n} T={T} fragment {f}")
        assert [r.shape[0] for r in got] == [int(d.sum()) for d in dones]
    # the members hold different fragments (one reading another's table entry would show)
    assert not np.array_equal(pairs[0][0].records_get(0), pairs[1][0].records_get(0))
    _close(group, pairs)


@pytest.mark.parametrize("n", [20, 65])
def test_shared_decentral_three_members(n):
    T = 17
    rng = np.random.default_rng(n)
    pairs = _pairs(C4, n, T, 3)
    assert pairs[0][0].layout[0]["C"] == 4 * n
    group = N.FinishGroup([c for c, _ in pairs])
    for f in range(2):
        _fragments(pairs, _random_dones(rng, 3, T, n), 7 * n + f)
        _run_and_compare(group, pairs, f"SharedDecentral n={n} fragment {f}")
    _close(group, pairs)


def test_members_that_differ_where_it_matters():
    n, T = 65, 17
    pairs = _pairs(LOCAL, n, T, 4)
    dones = [np.zeros((T, n), np.uint8) for _ in range(4)]
    # member 0: no done flag at all; 1: the first and the last step; 2: every env at one step;
    # 3: a few, so that the totals are all unequal
    dones[1][0, ::3] = 1
    dones[1][T - 1, 1::2] = 1
    dones[2][5] = 1
    dones[3][T // 2, [0, 63, 64]] = 1
    group = N.FinishGroup([c for c, _ in pairs])
    _fragments(pairs, dones, 3)
    got = _run_and_compare(group, pairs, "different members")
    counts = [r.shape[0] for r in got]
    assert counts == [int(d.sum()) for d in dones] and counts[0] == 0 and len(set(counts)) == 4
    assert (pairs[0][0].episodes_inflight()[:, 5] == T).all()   # the member without rows advanced its state
    # a second fragment with the roles rotated: every member's base and table are its own again
    dones = dones[1:] + dones[:1]
    _fragments(pairs, dones, 4)
    got = _run_and_compare(group, pairs, "different members, rotated")
    assert [r.shape[0] for r in got] == [int(d.sum()) for d in dones]
    _close(group, pairs)


def test_table_growth_of_one_member():
    n, T = 65, 17
    pairs = _pairs(LOCAL, n, T, 3)
    group = N.FinishGroup([c for c, _ in pairs])

    def scripted(counts):
        dones = [np.zeros((T, n), np.uint8) for _ in counts]
        for d, k in zip(dones, counts):
            d.reshape(-1)[np.linspace(0, T * n - 1, k).astype(int)] = 1
        return dones

    # first run: every table is sized to its count; second: member 0's count passes its cap (5 -> 40
    # rows: a new table), the others' stay below theirs; third: nothing grows
    for f, counts in enumerate([(5, 50, 50), (40, 10, 12), (7, 50, 3)]):
        dones = scripted(counts)
        assert [int(d.sum()) for d in dones] == list(counts)
        _fragments(pairs, dones, 20 + f)
        got = _run_and_compare(group, pairs, f"growth run {f}")
        assert [r.shape[0] for r in got] == list(counts)
    _close(group, pairs)


def test_one_member_equals_the_plain_path():
    n, T = 65, 33
    rng = np.random.default_rng(1)
    pairs = _pairs(LOCAL, n, T, 1)
    group = N.FinishGroup([pairs[0][0]])
    for f in range(2):
        _fragments(pairs, _random_dones(rng, 1, T, n), 30 + f)
        _run_and_compare(group, pairs, f"M=1 fragment {f}")
    _close(group, pairs)


def test_graphnet_members():
    n, T = 8, 17
    rng = np.random.default_rng(2)
    pairs = _pairs(GNN_ENV, n, T, 2)
    assert pairs[0][0].cfg.model_kind == N.MODEL_GNN
    group = N.FinishGroup([c for c, _ in pairs])
    for f in range(2):
        _fragments(pairs, _random_dones(rng, 2, T, n, 0.2), 40 + f)
        _run_and_compare(group, pairs, f"GraphNet fragment {f}")
    _close(group, pairs)


# ---- refusals -----------------------------------------------------------------------------------
def _refused(contexts, match):
    with pytest.raises(N.DdrlError, match=match):
        N.FinishGroup(contexts).close()


def test_create_refusals():
    import torch
    n, T = 8, 16
    a, b = _ctx(LOCAL, n, T, 0), _ctx(LOCAL, n, T, 1)
    lib = N.load()
    h = N.VP()
    with pytest.raises(N.DdrlError, match="finish group: at least one member is needed"):
        N.FinishGroup([])
    with pytest.raises(N.DdrlError, match="null argument"):
        N._ck(lib.ddrl_finish_group_create(None, 1, C.byref(h)))
    with pytest.raises(N.DdrlError, match="null argument"):
        N._ck(lib.ddrl_finish_group_create((N.VP * 1)(a.h), 1, None))
    with pytest.raises(N.DdrlError, match="finish group: member 1 is a null context"):
        N._ck(lib.ddrl_finish_group_create((N.VP * 2)(a.h, None), 2, C.byref(h)))
    _refused([a, b, a], "finish group: member 2 repeats member 0")
    side = torch.cuda.Stream()
    b.set_stream(side.cuda_stream)
    _refused([a, b], "finish group: member 1 is on another stream than member 0")
    b.set_stream(torch.cuda.current_stream().cuda_stream)
    for other, field in ((_ctx(LOCAL, n, T + 1, 2), "frag_len"), (_ctx(LOCAL, n + 1, T, 2), "n_envs"),
                         (_ctx(LOCAL, n, T, 2, {"gamma": 0.9}), "gamma"),
                         (_ctx(LOCAL, n, T, 2, cfg_set={"agent_policy": (N.i32 * N.MAX_AG)(1, 0, 2, 3)}), "agent_policy"),
                         (_ctx(C4, n, T, 2), "n_policies")):
        _refused([a, b, other], f"finish group: member 2 differs from member 0 in {field}")
        other.close()
    N.FinishGroup([a, b]).close()   # and what is equal in all of that is accepted
    a.close()
    b.close()


def test_run_and_rows_refusals_leave_every_member_untouched():
    import torch
    n, T = 65, 17
    rng = np.random.default_rng(3)
    pairs = _pairs(LOCAL, n, T, 3)
    members = [c for c, _ in pairs]
    group = N.FinishGroup(members)
    lib = N.load()
    _fragments(pairs, _random_dones(rng, 3, T, n), 50)
    before = [[c.records_get(p) for p in range(c.cfg.n_policies)] + [c.episodes_inflight()] for c in members]
    # member 1 has been finished by its own calls: the whole run is refused, nothing is launched
    rows1 = _plain(members[1])
    with pytest.raises(N.DdrlError, match="finish group: member 1: this fragment has been collected"):
        group.run()
    for m in (0, 2):
        after = [members[m].records_get(p) for p in range(members[m].cfg.n_policies)] + [members[m].episodes_inflight()]
        for x, y in zip(before[m], after):
            np.testing.assert_array_equal(x, y)
    # ... so the plain path on the others, afterwards, still gives the twins' results
    got = [_plain(members[0]), rows1, _plain(members[2])]
    for m, (c, t) in enumerate(pairs):
        _assert_same_member(c, t, got[m], _plain(t), f"after the refusal, member {m}")
    # null arguments, a wrong row count, another stream
    with pytest.raises(N.DdrlError, match="null finish group"):
        N._ck(lib.ddrl_finish_group_run(None, (C.c_int64 * 3)()))
    with pytest.raises(N.DdrlError, match="finish group: null count output"):
        N._ck(lib.ddrl_finish_group_run(group.h, None))
    _fragments(pairs, _random_dones(rng, 3, T, n), 51)
    side = torch.cuda.Stream()
    members[2].set_stream(side.cuda_stream)
    with pytest.raises(N.DdrlError, match="finish group: member 2 is on another stream than member 0"):
        group.run()
    members[2].set_stream(torch.cuda.current_stream().cuda_stream)
    counts = (C.c_int64 * 3)()
    N._ck(lib.ddrl_finish_group_run(group.h, counts))
    assert min(counts) > 0
    bufs = [np.empty((int(k) + 1, 8)) for k in counts]
    ptrs = (N.VP * 3)(*[b.ctypes.data for b in bufs])
    with pytest.raises(N.DdrlError, match="finish group: null rows argument"):
        N._ck(lib.ddrl_finish_group_rows(group.h, None, counts))
    with pytest.raises(N.DdrlError, match="finish group: null rows argument"):
        N._ck(lib.ddrl_finish_group_rows(group.h, ptrs, None))
    wrong = (C.c_int64 * 3)(counts[0], counts[1] + 1, counts[2])
    with pytest.raises(N.DdrlError, match="finish group: member 1: n_rows differs from the last collect's count"):
        N._ck(lib.ddrl_finish_group_rows(group.h, ptrs, wrong))
    N._ck(lib.ddrl_finish_group_rows(group.h, ptrs, counts))
    for m, (c, t) in enumerate(pairs):
        _assert_same_member(c, t, bufs[m][:counts[m]], _plain(t), f"rows by hand, member {m}")
    # the "collected once" refusal holds after a group run, on the group and on the member
    with pytest.raises(N.DdrlError, match="finish group: member 0: this fragment has been collected"):
        group.run()
    with pytest.raises(N.DdrlError, match="this fragment has been collected"):
        members[2].episodes_collect()
    group.close()
    with pytest.raises(N.DdrlError, match="used after close"):
        group.run()
    _close(group, pairs)


# ---- what follows the finish --------------------------------------------------------------------
def _schedule(ctx, T, epochs, seed):
    import torch
    rng = np.random.default_rng(seed)
    sh, pe = [], []
    for p in range(ctx.cfg.n_policies):
        R = T * ctx.layout[p]["C"]
        sh.append(torch.from_numpy(rng.permutation(R).astype(np.int32)).cuda())
        pe.append(torch.from_numpy(np.stack([rng.permutation(R // 128) for _ in range(epochs)]).astype(np.int32)).cuda())
    return sh, pe, [float(k) for k in rng.uniform(0.1, 0.5, ctx.cfg.n_policies)]


def _updated(n, T, epochs, M):
    """M pairs after a group finish + group update (members) and gae + ppo_update (twins)."""
    rng = np.random.default_rng(4)
    pairs = _pairs(LOCAL, n, T, M, {"num_sgd_iter": epochs})
    members = [c for c, _ in pairs]
    finish, update = N.FinishGroup(members), N.UpdateGroup(members)
    _fragments(pairs, _random_dones(rng, M, T, n), 60)
    finish.run()
    scheds = [_schedule(c, T, epochs, 70 + m) for m, c in enumerate(members)]
    update.run([s[0] for s in scheds], [s[1] for s in scheds], [s[2] for s in scheds])
    update.finish()
    for (c, t), (sh, pe, kl) in zip(pairs, scheds):
        t.gae()
        t.ppo_update((1 << t.cfg.n_policies) - 1, sh, pe, kl)
        t.synchronize()
    return pairs, finish, update


def test_a_following_group_update_equals_the_twins():
    n, T = 8, 16   # 128 rows per policy: one minibatch, one epoch
    pairs, finish, update = _updated(n, T, 1, 3)
    for m, (c, t) in enumerate(pairs):
        for p in range(c.cfg.n_policies):
            np.testing.assert_array_equal(c.params_get(p), t.params_get(p), err_msg=f"member {m} policy {p} theta")
            for x, y in zip(c.adam_get(p), t.adam_get(p)):
                np.testing.assert_array_equal(x, y, err_msg=f"member {m} policy {p} Adam state")
    assert not np.array_equal(pairs[0][0].params_get(0), pairs[1][0].params_get(0))
    update.close()
    _close(finish, pairs)


def test_stats_range_equals_the_members_own_readback():
    n, T, epochs = 8, 32, 2   # 256 rows per policy: 2 minibatches x 2 epochs = 4 statistics rows
    pairs, finish, update = _updated(n, T, epochs, 3)
    P = pairs[0][0].cfg.n_policies
    for first, steps in ((0, 4), (2, 2), (3, 1), (1, 2), (4, 0)):
        got = update.stats_range(first, steps)
        assert got.dtype == np.float32 and got.shape == (3, P, steps, 8)
        for m, (c, t) in enumerate(pairs):
            for p in range(P):
                np.testing.assert_array_equal(got[m, p], c.ppo_stats(p, steps, first), err_msg=f"member {m} policy {p}")
                np.testing.assert_array_equal(got[m, p], t.ppo_stats(p, steps, first), err_msg=f"twin {m} policy {p}")
    assert np.isfinite(update.stats_range(0, 4)).all()
    for first, steps in ((3, 2), (5, 0), (0, 5)):
        with pytest.raises(N.DdrlError, match="update group: member 0, policy 0: more stats requested than the schedule holds"):
            update.stats_range(first, steps)
    with pytest.raises(N.DdrlError, match="null update group"):
        N._ck(N.load().ddrl_update_group_stats_range(None, 0, 1, None))
    with pytest.raises(N.DdrlError, match="null stats buffer"):
        N._ck(N.load().ddrl_update_group_stats_range(update.h, 0, 1, None))
    update.close()
    _close(finish, pairs)
