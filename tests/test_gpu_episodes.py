"""On-device episode accounting of the training rollout (ddrl_episodes_*; episodes.hip) against
tests/episodes_reference.py, the plain-Python loop of RLlib 1.0's MultiAgentEpisode.

Rewards go through the ordinary ddrl_reward calls with scripted done flags; the fp32 `rew` column
is read back with records_get and the checker sums it in fp64 in (t, env, agent) order.  The
device does the same fp64 additions in the same order, so every row field and the in-flight
state are compared with assert_array_equal: there is no tolerance.

Shapes: N in {3, 64, 65, 130} (below a wave, one wave, a ragged second, a ragged third) and
T in {1, U - 1, U, U + 1, 2 U + 1} with U = 16, the walk's load chunk."""
import numpy as np
import pytest

from ddrl_amd import native as N
from tests import episodes_reference as R
from tests.gpu_harness import dev, init_params, make_ctx

pytestmark = pytest.mark.gpu
U = 16
LOCAL = "QuantrupedMultiEnv_Local"
ENVS = {"centralized": "QuantrupedMultiEnv_Centralized", "twosides": "QuantrupedMultiEnv_TwoSides",
        "local": LOCAL, "shared": "QuantrupedMultiEnv_SharedDecentral"}


def _drive(ctx, cfg, rng, done, steps=None):
    """Rewards of the steps (all by default) through ddrl_reward with the scripted done flags."""
    T, n = done.shape
    actions = dev(rng.uniform(-1, 1, size=(n, 8)).astype(np.float32))
    for t in (range(T) if steps is None else steps):
        fw = dev(rng.normal(size=n).astype(np.float32))
        cfrc = dev((rng.normal(size=(n, 14, 6)) * 1.5).astype(np.float32))
        ctx.reward(t, fw, cfrc, actions, dev(done[t]))


def _collect_and_check(ctx, cfg, ref, done):
    want = ref.fragment(R.record_rewards(ctx, cfg), done)
    got = ctx.episodes_collect()
    assert got.dtype == np.float64 and got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(ctx.episodes_inflight(), ref.inflight())
    return got


def _fresh(env, n, T):
    ctx, cfg, _ = make_ctx(env, n, T)
    return ctx, cfg, R.EpisodeReference(n, cfg.n_agents)


@pytest.mark.parametrize("T", [1, U - 1, U, U + 1, 2 * U + 1])
@pytest.mark.parametrize("n", [3, 64, 65, 130])
def test_random_dones_every_shape_local(n, T):
    rng = np.random.default_rng(100 * n + T)
    ctx, cfg, ref = _fresh(LOCAL, n, T)
    for _ in range(2):   # the second fragment starts from a non-zero in-flight state
        done = (rng.random(size=(T, n)) < 0.1).astype(np.uint8)
        _drive(ctx, cfg, rng, done)
        got = _collect_and_check(ctx, cfg, ref, done)
        assert got.shape[0] == int(done.sum())
    ctx.close()


@pytest.mark.parametrize("name", list(ENVS))
def test_every_architecture(name):
    n, T = 65, 2 * U + 1
    rng = np.random.default_rng(7)
    ctx, cfg, ref = _fresh(ENVS[name], n, T)
    assert cfg.n_agents == {"centralized": 1, "twosides": 2, "local": 4, "shared": 4}[name]
    for _ in range(2):
        done = (rng.random(size=(T, n)) < 0.1).astype(np.uint8)
        _drive(ctx, cfg, rng, done)
        got = _collect_and_check(ctx, cfg, ref, done)
        assert got.shape[0] > 0
        # agents the env does not have are NaN, the others finite
        assert np.isnan(got[:, 4 + cfg.n_agents:]).all() and np.isfinite(got[:, :4 + cfg.n_agents]).all()
    ctx.close()


def _pattern(name, n, T, rng):
    done = np.zeros((T, n), np.uint8)
    if name == "same_step":          # every env at the same step: full-wave ballots
        done[5] = 1
    elif name == "first_and_last":   # t = 0 and t = T - 1
        done[0, ::3] = 1
        done[T - 1, 1::2] = 1
    elif name == "consecutive":      # length-1 episodes
        done[4:9, [0, 1, n // 2, n - 1]] = 1
        done[T - 3:, 2] = 1
    elif name == "last_lane":        # one env only, in the last wave's last lane
        done[T // 2, n - 1] = 1
    else:
        assert name == "none"
    return done


@pytest.mark.parametrize("name,n,T", [("none", 65, U + 1), ("same_step", 130, U + 1), ("first_and_last", 65, 2 * U + 1),
                                      ("consecutive", 65, U + 1), ("last_lane", 130, U + 1), ("last_lane", 64, U)])
def test_scripted_done_patterns(name, n, T):
    rng = np.random.default_rng(11)
    ctx, cfg, ref = _fresh(LOCAL, n, T)
    done = _pattern(name, n, T, rng)
    _drive(ctx, cfg, rng, done)
    got = _collect_and_check(ctx, cfg, ref, done)
    assert got.shape == (int(done.sum()), 8)
    if name == "none":
        assert got.shape[0] == 0
        assert (ctx.episodes_inflight()[:, 5] == T).all()          # state advanced
    if name == "consecutive":
        assert (got[:, 2] == 1).sum() >= 4 * 4
    # rows in ascending (t, env) order
    key = got[:, 0] * n + got[:, 1]
    assert (np.diff(key) > 0).all()
    ctx.close()


def test_episodes_span_fragments_and_reset_drops_them():
    n, T = 65, U + 1
    rng = np.random.default_rng(5)
    ctx, cfg, ref = _fresh(LOCAL, n, T)
    seen = []
    for f in range(4):
        done = (rng.random(size=(T, n)) < 0.02).astype(np.uint8)
        done[:, [0, 1, n - 1]] = 0
        if f == 1:
            done[3, 0] = 1          # env 0: an episode over two fragments
        if f == 2:
            done[5, 1] = 1          # env 1: over three
        _drive(ctx, cfg, rng, done)
        seen.append(_collect_and_check(ctx, cfg, ref, done))
    row0 = seen[1][(seen[1][:, 1] == 0)]
    row1 = seen[2][(seen[2][:, 1] == 1)]
    assert row0.shape[0] == 1 and row0[0, 2] == T + 4
    assert row1.shape[0] == 1 and row1[0, 2] == 2 * T + 6
    infl = ctx.episodes_inflight()
    assert infl[n - 1, 5] == 4 * T and infl[n - 1, 0] != 0.0         # the env that never finishes
    ctx.episodes_reset()
    np.testing.assert_array_equal(ctx.episodes_inflight(), np.zeros((n, 6)))
    ref.reset()
    done = (rng.random(size=(T, n)) < 0.1).astype(np.uint8)
    _drive(ctx, cfg, rng, done)
    _collect_and_check(ctx, cfg, ref, done)
    ctx.close()


def test_table_growth():
    n, T = 65, U + 1
    rng = np.random.default_rng(9)
    ctx, cfg, ref = _fresh(LOCAL, n, T)
    for k in range(3):
        done = np.zeros((T, n), np.uint8)
        if k == 0:
            done[2, 7] = done[9, 64] = 1
        elif k == 1:
            done = (rng.random(size=(T, n)) < 0.7).astype(np.uint8)
            assert done.sum() > n * T // 2
        else:
            done[T - 1, 33] = 1
        _drive(ctx, cfg, rng, done)
        got = _collect_and_check(ctx, cfg, ref, done)
        assert got.shape[0] == int(done.sum())
    ctx.close()


def test_fp64_sums_of_fp32_rewards():
    """Rewards of about 1e4 and about 1e-3 in one episode: an fp32 running sum drops the small
    ones, the fp64 sum keeps them; the interleaved total is not the sum of the agent totals."""
    n, T = 65, 2 * U + 1
    rng = np.random.default_rng(13)
    ctx, cfg, ref = _fresh(LOCAL, n, T)
    done = (rng.random(size=(T, n)) < 0.05).astype(np.uint8)
    done[T - 1] = 1
    _drive(ctx, cfg, rng, done)
    recs = [ctx.records_get(p) for p in range(cfg.n_policies)]
    for p, rec in enumerate(recs):
        big = rng.random(size=rec.shape[0]) < 0.3
        rec[:, ctx.layout[p]["rew"]] = np.where(big, rng.normal(size=rec.shape[0]) * 1e4,
                                                rng.normal(size=rec.shape[0]) * 1e-3).astype(np.float32)
        ctx.records_set(p, rec)
    rew = R.record_rewards(ctx, cfg, recs)
    got = _collect_and_check(ctx, cfg, ref, done)
    # the inputs do tell fp32 from fp64 accumulation, and interleaved from per-agent sums
    run32 = np.zeros(n, np.float32)
    differs = 0
    for t in range(T):
        for j in range(cfg.n_agents):
            run32 = (run32 + rew[t, :, j]).astype(np.float32)
        for e in np.nonzero(done[t])[0]:
            row = got[(got[:, 0] == t) & (got[:, 1] == e)][0]
            differs += float(run32[e]) != row[3]
            run32[e] = 0
    assert differs > got.shape[0] // 2
    assert (got[:, 3] != got[:, 4:8].sum(axis=1)).any()
    ctx.close()


def test_collect_once_and_argument_errors():
    import ctypes as C
    n, T = 3, U - 1
    rng = np.random.default_rng(17)
    ctx, cfg, ref = _fresh(LOCAL, n, T)
    buf = np.zeros((4, 8))
    assert ctx.lib.ddrl_episodes_rows(ctx.h, buf.ctypes.data, 0) != 0            # before any collect
    assert b"collect first" in ctx.lib.ddrl_last_error()
    done = (rng.random(size=(T, n)) < 0.3).astype(np.uint8)
    _drive(ctx, cfg, rng, done)
    got = _collect_and_check(ctx, cfg, ref, done)
    with pytest.raises(N.DdrlError, match="has been collected"):
        ctx.episodes_collect()
    np.testing.assert_array_equal(ctx.episodes_inflight(), ref.inflight())       # the refused call walked nothing
    assert ctx.lib.ddrl_episodes_rows(ctx.h, buf.ctypes.data, got.shape[0] + 1) != 0
    assert b"n_rows" in ctx.lib.ddrl_last_error()
    assert ctx.lib.ddrl_episodes_rows(ctx.h, None, got.shape[0]) != 0
    assert b"null" in ctx.lib.ddrl_last_error()
    assert ctx.lib.ddrl_episodes_collect(ctx.h, None) != 0
    assert b"null" in ctx.lib.ddrl_last_error()
    assert ctx.lib.ddrl_episodes_inflight(ctx.h, None, n) != 0
    assert b"null" in ctx.lib.ddrl_last_error()
    assert ctx.lib.ddrl_episodes_inflight(ctx.h, buf.ctypes.data, n + 1) != 0
    assert ctx.lib.ddrl_episodes_reset(None) != 0
    assert b"null context" in ctx.lib.ddrl_last_error()
    nf = C.c_int64()
    assert ctx.lib.ddrl_episodes_collect(None, C.byref(nf)) != 0
    # one more reward call re-arms the fragment: the walk goes over all of it again
    _drive(ctx, cfg, rng, done, steps=[T - 1])
    _collect_and_check(ctx, cfg, ref, done)
    ctx.close()


def _rollout(ctx, cfg, rng, T, done):
    import torch
    n = cfg.n_envs
    actions = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    ctx.observe(dev((rng.normal(size=(n, cfg.obs_full_dim)) * 2 + 0.5).astype(np.float32)))
    for t in range(T):
        ctx.act(t, dev(rng.normal(size=(n, cfg.n_agents, cfg.act_dim)).astype(np.float32)), actions)
        ctx.reward(t, dev(rng.normal(size=n).astype(np.float32)),
                   dev((rng.normal(size=(n, 14, 6)) * 1.5).astype(np.float32)), actions, dev(done[t]))
        ctx.observe(dev((rng.normal(size=(n, cfg.obs_full_dim)) * 2 + 0.5).astype(np.float32)))
    ctx.bootstrap()


def _state(ctx, cfg):
    out = {"filter": np.concatenate([[ctx.filter_get()[0]], *ctx.filter_get()[1:]])}
    for p in range(cfg.n_policies):
        m, v, b1, b2 = ctx.adam_get(p)
        out.update({f"rec{p}": ctx.records_get(p), f"last_v{p}": ctx.last_values_get(p), f"theta{p}": ctx.params_get(p),
                    f"m{p}": m, f"v{p}": v, f"beta{p}": np.array([b1, b2]), f"adv_norm{p}": ctx.adv_norm_get(p)})
    return out


def test_collect_leaves_training_alone():
    """A context that collects and its twin that never does: records, GAE output, filters,
    parameters and Adam state stay bit-identical, also after gae and a 20-step update."""
    n, T = 65, 2 * U + 1
    done = (np.random.default_rng(3).random(size=(T, n)) < 0.1).astype(np.uint8)
    ctxs = []
    for _ in range(2):
        ctx, cfg, _inst = make_ctx(LOCAL, n, T)
        init_params(ctx, cfg, 21, head_scale=1.0)
        _rollout(ctx, cfg, np.random.default_rng(4), T, done)
        ctxs.append(ctx)
    a, b = ctxs
    ref = R.EpisodeReference(n, cfg.n_agents)
    got = _collect_and_check(a, cfg, ref, done)
    assert got.shape[0] == int(done.sum())

    def same(tag):
        sa, sb = _state(a, cfg), _state(b, cfg)
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"{tag}: {k}")
    same("after collect")
    a.gae()
    b.gae()
    same("after gae")
    srng = np.random.default_rng(8)
    P = cfg.n_policies
    sh, pe = [], []
    for p in range(P):
        Rr = T * a.layout[p]["C"]
        nb = max(1, Rr // cfg.sgd_minibatch_size)
        sh.append(dev(srng.permutation(Rr).astype(np.int32)))
        pe.append(dev(np.stack([srng.permutation(nb) for _ in range(cfg.num_sgd_iter)]).astype(np.int32)))
    for ctx in (a, b):
        ctx.ppo_update((1 << P) - 1, sh, pe, [0.2] * P, max_steps=20)
        ctx.synchronize()
    same("after update")
    for p in range(P):
        np.testing.assert_array_equal(a.ppo_stats(p, 20), b.ppo_stats(p, 20))
        assert not np.array_equal(a.params_get(p), init_theta(cfg, p))
    a.close()
    b.close()


def init_theta(cfg, p):
    from oracle import ddrl_oracle as O
    from tests.gpu_harness import make_params
    return O.pack(make_params(cfg, 21, 1.0)[p], O.ffn_param_shapes(cfg.obs_dim[p], 2 * cfg.act_dim))
