"""The device generator (csrc/rng.hip) against its numpy restatement (tests/rng_oracle.py, written
from DESIGN.md section 3 "Device randomness"): the noise values and their invariances, the
distribution, the schedules, and the trainers with rng_backend "device" (needs an MI355X)."""
import numpy as np
import pytest

import rng_oracle as O

pytestmark = pytest.mark.gpu
LOCAL, CENTRAL, C4 = "QuantrupedMultiEnv_Local", "QuantrupedMultiEnv_Centralized", "QuantrupedMultiEnv_SharedDecentral"
SEED = 0x9E3779B97F4A7C15   # a seed with both 32-bit halves in use


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ctx(env, n_envs, T=4, config=None):
    from gpu_harness import make_ctx
    ctx, cfg, _ = make_ctx(env, n_envs, T, config)
    return ctx, cfg


def _slab(cfg, n_steps):
    import torch
    return torch.full((n_steps, cfg.n_envs, cfg.n_agents, cfg.act_dim), float("nan"), dtype=torch.float32, device="cuda")


def _fill(ctx, cfg, n_steps):
    import torch
    eps = _slab(cfg, n_steps)
    ctx.noise_fill(n_steps, eps)
    torch.cuda.synchronize()
    return eps.cpu().numpy()


# ---- 1. noise against the oracle ----
@pytest.mark.parametrize("env,n_envs,n_steps", [(LOCAL, 5, 3), (CENTRAL, 33, 1), (LOCAL, 300, 7)],
                         ids=["local-5x3", "central-33", "local-300x7"])
def test_noise_matches_the_oracle(env, n_envs, n_steps):
    """Against the fp64 evaluation of the same formula.  The bound is 4 x the largest error of the
    numpy fp32 restatement against fp64 over the same samples (the margin covers the device's log,
    sqrt, sin and cos); a wrong word is off by O(1)."""
    from ddrl_amd import native as N
    ctx, cfg = _ctx(env, n_envs)
    pos = (1 << 32) - 2   # the absolute step crosses into the counter's second word
    ctx.rng_state_set(N.RNG_NOISE, SEED, pos)
    got = _fill(ctx, cfg, n_steps)
    assert ctx.rng_state(N.RNG_NOISE) == (SEED, pos + n_steps)
    ref = O.noise(SEED, pos, n_steps, n_envs, cfg.n_agents, cfg.act_dim, np.float64)
    ref32 = O.noise(SEED, pos, n_steps, n_envs, cfg.n_agents, cfg.act_dim, np.float32)
    bound = 4.0 * np.abs(ref32.astype(np.float64) - ref).max()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"max |device - fp64| {err:.3e}, bound {bound:.3e} (4 x the fp32 restatement's)")
    assert np.isfinite(got).all()
    assert err <= bound
    ctx.close()


# ---- 2. invariances, all bitwise ----
def test_noise_chunks_rewind_and_env_count():
    from ddrl_amd import native as N
    a, cfg_a = _ctx(LOCAL, 5)
    b, cfg_b = _ctx(LOCAL, 9)
    for c in (a, b):
        c.rng_seed(N.RNG_NOISE, SEED)
    whole = _fill(a, cfg_a, 7)
    assert a.rng_state(N.RNG_NOISE) == (SEED, 7)
    a.rng_state_set(N.RNG_NOISE, SEED, 0)           # state_set rewinds the stream
    first, rest = _fill(a, cfg_a, 3), _fill(a, cfg_a, 4)
    np.testing.assert_array_equal(np.concatenate([first, rest]), whole)
    a.rng_state_set(N.RNG_NOISE, SEED, 3)
    np.testing.assert_array_equal(_fill(a, cfg_a, 4), whole[3:])
    np.testing.assert_array_equal(_fill(b, cfg_b, 7)[:, :5], whole)   # env e does not depend on N
    a.rng_seed(N.RNG_NOISE, SEED + 1)
    assert not np.array_equal(_fill(a, cfg_a, 7), whole)
    a.close(), b.close()


def test_noise_group_equals_solo_fills():
    import torch
    from ddrl_amd import native as N
    seeds = (SEED, 1, 2 ** 40 + 3)
    ctxs = [_ctx(LOCAL, 300, T=2) for _ in seeds]
    cfg = ctxs[0][1]
    solo = []
    for (c, _), s in zip(ctxs, seeds):
        c.rng_state_set(N.RNG_NOISE, s, 11)
        solo.append(_fill(c, cfg, 3))
        c.rng_state_set(N.RNG_NOISE, s, 11)
    slabs = [_slab(cfg, 3) for _ in seeds]
    N.noise_fill_group([c for c, _ in ctxs], 3, slabs)
    torch.cuda.synchronize()
    for m, ((c, _), s) in enumerate(zip(ctxs, seeds)):
        np.testing.assert_array_equal(slabs[m].cpu().numpy(), solo[m], err_msg=f"member {m}")
        assert c.rng_state(N.RNG_NOISE) == (s, 14)
    assert not np.array_equal(solo[0], solo[1])
    # a second, smaller and a larger group on the same leading member reuse / grow its table
    N.noise_fill_group([ctxs[0][0]], 3, slabs[:1])
    more = [_ctx(LOCAL, 300, T=2)[0] for _ in range(2)]
    for c in more:
        c.rng_seed(N.RNG_NOISE, 5)
    N.noise_fill_group([c for c, _ in ctxs] + more, 3, slabs + [_slab(cfg, 3), _slab(cfg, 3)])
    torch.cuda.synchronize()
    assert ctxs[0][0].rng_state(N.RNG_NOISE) == (seeds[0], 20)
    for c in [c for c, _ in ctxs] + more:
        c.close()


# ---- 3. distribution ----
def test_noise_distribution():
    """2^20 normals: mean, variance, fourth moment and the lag-1 correlations along the step and the
    env axis within 5 standard errors (1 / sqrt n, sqrt(2 / n), sqrt(96 / n), 1 / sqrt n)."""
    from ddrl_amd import native as N
    ctx, cfg = _ctx(LOCAL, 1024)
    ctx.rng_seed(N.RNG_NOISE, 20260101)
    z = _fill(ctx, cfg, 128).astype(np.float64).reshape(128, 1024, 8)
    n = z.size
    assert n == 1 << 20
    stats = {"mean": (z.mean(), 0.0, 1 / np.sqrt(n)), "variance": (z.var(), 1.0, np.sqrt(2 / n)),
             "fourth moment": ((z ** 4).mean(), 3.0, np.sqrt(96 / n)),
             "lag-1 along step": ((z[1:] * z[:-1]).mean(), 0.0, 1 / np.sqrt(z[1:].size)),
             "lag-1 along env": ((z[:, 1:] * z[:, :-1]).mean(), 0.0, 1 / np.sqrt(z[:, 1:].size))}
    for name, (got, want, se) in stats.items():
        print(f"{name}: {got:.6f} ({(got - want) / se:+.2f} standard errors)")
    for name, (got, want, se) in stats.items():
        assert abs(got - want) <= 5 * se, name
    ctx.close()


# ---- 4. schedules ----
SCHEDULES = [(LOCAL, 8, 48), (LOCAL, 5, 30), (LOCAL, 8, 128), (LOCAL, 5, 205), (C4, 2, 64)]


def _schedule(ctx):
    import torch
    sh, pe = ctx.schedule_alloc()
    for x in sh + pe:
        x.fill_(-7)
    ctx.schedule_fill(sh, pe)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in sh], [x.cpu().numpy() for x in pe]


def _oracle_schedule(ctx, cfg, seed, draw):
    out_sh, out_pe = [], []
    for p in range(cfg.n_policies):
        R = cfg.frag_len * ctx.layout[p]["C"]
        sh, pe = O.schedule(seed, draw, p, R, max(1, R // cfg.sgd_minibatch_size), cfg.num_sgd_iter)
        out_sh.append(sh), out_pe.append(pe)
    return out_sh, out_pe


@pytest.mark.parametrize("env,n_envs,T", SCHEDULES, ids=[f"{e.split('_')[-1]}-{n}x{t}" for e, n, t in SCHEDULES])
def test_schedules_match_the_oracle(env, n_envs, T):
    from ddrl_amd import native as N
    ctx, cfg = _ctx(env, n_envs, T, {"num_sgd_iter": 3})
    R = T * ctx.layout[0]["C"]
    assert R == {(8, 48): 384, (5, 30): 150, (8, 128): 1024, (5, 205): 1025, (2, 64): 512}[(n_envs, T)]
    ctx.rng_state_set(N.RNG_SCHEDULE, SEED, (1 << 32) - 1)
    for draw in ((1 << 32) - 1, 1 << 32):   # two draws: the index advances by one per fill, across the word
        assert ctx.rng_state(N.RNG_SCHEDULE) == (SEED, draw)
        sh, pe = _schedule(ctx)
        ref_sh, ref_pe = _oracle_schedule(ctx, cfg, SEED, draw)
        for p in range(cfg.n_policies):
            np.testing.assert_array_equal(sh[p], ref_sh[p], err_msg=f"shuffle of policy {p}, draw {draw}")
            np.testing.assert_array_equal(pe[p], ref_pe[p], err_msg=f"perm of policy {p}, draw {draw}")
            assert np.array_equal(np.sort(sh[p]), np.arange(R))
    ctx.close()


def test_schedules_differ_and_mask():
    import torch
    from ddrl_amd import native as N
    ctx, cfg = _ctx(LOCAL, 8, 48, {"num_sgd_iter": 3})
    ctx.rng_seed(N.RNG_SCHEDULE, 3)
    sh0, pe0 = _schedule(ctx)
    sh1, pe1 = _schedule(ctx)
    assert not np.array_equal(sh0[0], sh1[0]) and not np.array_equal(pe0[0], pe1[0])        # draws
    assert not np.array_equal(sh0[0], sh0[1]) and not np.array_equal(sh0[2], sh0[3])        # policies
    assert not np.array_equal(pe0[0][0], pe0[0][1]) or not np.array_equal(pe0[0][1], pe0[0][2])   # epochs (nb = 3)
    # a mask fills its policies only, with the values of the full fill of the same draw
    ctx.rng_state_set(N.RNG_SCHEDULE, 3, 0)
    sh, pe = ctx.schedule_alloc()
    for x in sh + pe:
        x.fill_(-7)
    ctx.schedule_fill(sh, pe, mask=0b0101)
    torch.cuda.synchronize()
    for p in range(4):
        want_sh, want_pe = (sh0[p], pe0[p]) if p in (0, 2) else (np.full_like(sh0[p], -7), np.full_like(pe0[p], -7))
        np.testing.assert_array_equal(sh[p].cpu().numpy(), want_sh)
        np.testing.assert_array_equal(pe[p].cpu().numpy(), want_pe)
    ctx.close()


def test_schedule_group_equals_solo_fills():
    import torch
    from ddrl_amd import native as N
    seeds = (3, 4, SEED)
    ctxs = [_ctx(LOCAL, 5, 205, {"num_sgd_iter": 2})[0] for _ in seeds]
    solo = []
    for c, s in zip(ctxs, seeds):
        c.rng_state_set(N.RNG_SCHEDULE, s, 9)
        solo.append(_schedule(c))
        c.rng_state_set(N.RNG_SCHEDULE, s, 9)
    arrays = [c.schedule_alloc() for c in ctxs]
    N.schedule_fill_group(ctxs, [a[0] for a in arrays], [a[1] for a in arrays])
    torch.cuda.synchronize()
    for m, c in enumerate(ctxs):
        for p in range(4):
            np.testing.assert_array_equal(arrays[m][0][p].cpu().numpy(), solo[m][0][p], err_msg=f"member {m} shuffle {p}")
            np.testing.assert_array_equal(arrays[m][1][p].cpu().numpy(), solo[m][1][p], err_msg=f"member {m} perm {p}")
        assert c.rng_state(N.RNG_SCHEDULE) == (seeds[m], 10)
    assert not np.array_equal(solo[0][0][0], solo[1][0][0])   # members
    for c in ctxs:
        c.close()


def test_update_runs_over_filled_schedules():
    """A fused update over device-drawn schedules: the trainer's own path, statistics finite."""
    import torch
    from ddrl_amd import native as N
    from ddrl_amd.trainer import PPOTrainer
    tr = PPOTrainer({"env": LOCAL, "rollout_fragment_length": 48, "num_sgd_iter": 2, "rng_backend": "device"},
                    n_envs=8, seed=1)
    tr._sample()
    seed, draw = tr.ctx.rng_state(N.RNG_SCHEDULE)
    assert (seed, draw) == (1 + 7919, 0)
    sh, pe, nbs = tr._learn_schedules()
    assert nbs == [3] * 4
    tr.ctx.ppo_update(0b1111, sh, pe, tr.kl_coeff)
    torch.cuda.synchronize()
    ref_sh, ref_pe = _oracle_schedule(tr.ctx, tr.cfg, seed, draw)
    for p in range(4):
        np.testing.assert_array_equal(sh[p].cpu().numpy(), ref_sh[p])
        np.testing.assert_array_equal(pe[p].cpu().numpy(), ref_pe[p])
        assert np.isfinite(tr.ctx.ppo_stats(p, 2 * 3)).all()
    assert tr.ctx.rng_state(N.RNG_SCHEDULE) == (seed, 1)
    tr.stop()


def test_refusals():
    import torch
    from ddrl_amd import native as N
    a, cfg = _ctx(LOCAL, 5, 30)
    b, _ = _ctx(LOCAL, 9, 30)
    eps = _slab(cfg, 2)
    sh, pe = a.schedule_alloc()
    with pytest.raises(N.DdrlError, match="noise stream has no seed"):
        a.noise_fill(2, eps)
    with pytest.raises(N.DdrlError, match="schedule stream has no seed"):
        a.schedule_fill(sh, pe)
    with pytest.raises(N.DdrlError, match="no seed"):
        a.rng_state(N.RNG_NOISE)
    with pytest.raises(N.DdrlError, match="stream must be"):
        a.rng_seed(2, 0)
    for c in (a, b):
        c.rng_seed(N.RNG_NOISE, 1), c.rng_seed(N.RNG_SCHEDULE, 1)
    with pytest.raises(N.DdrlError, match="n_steps must be >= 1"):
        a.noise_fill(0, eps)
    with pytest.raises(N.DdrlError, match="null noise buffer"):
        a.noise_fill(2, None)
    with pytest.raises(N.DdrlError, match="16-byte aligned"):
        a.noise_fill(1, eps.view(-1)[1:1 + 5 * 8])
    with pytest.raises(N.DdrlError, match="outside the context"):
        a.schedule_fill(sh, pe, mask=0b10001)
    with pytest.raises(N.DdrlError, match="null schedule buffer of policy 2"):
        a.schedule_fill(sh[:2], pe)
    with pytest.raises(N.DdrlError, match="member 1 differs from member 0 in n_envs"):
        N.noise_fill_group([a, b], 2, [eps, eps])
    with pytest.raises(N.DdrlError, match="member 1 repeats member 0"):
        N.noise_fill_group([a, a], 2, [eps, eps])
    with pytest.raises(N.DdrlError, match="member 1 differs from member 0 in the rows"):
        N.schedule_fill_group([a, b], [sh, sh], [pe, pe])
    assert a.rng_state(N.RNG_NOISE) == (1, 0) and a.rng_state(N.RNG_SCHEDULE) == (1, 0)   # a refusal draws nothing
    torch.cuda.synchronize()
    a.close(), b.close()


# ---- 5. trainers ----
CONFIG = {"env": LOCAL, "env_backend": "device", "rng_backend": "device", "rollout_fragment_length": 32, "num_sgd_iter": 2}
SEEDS = (0, 1, 2)
UNTIMED = lambda r: {k: v for k, v in r.items() if k != "timers"}


def _same(a, b, what):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), f"{what}: keys {list(a)} != {list(b)}"
        for k in a:
            _same(a[k], b[k], f"{what}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


def _trainer_state(t):
    from ddrl_amd import native as N
    out = {"weights": t.get_weights(), "kl": list(t.kl_coeff), "filter": list(t.ctx.filter_get()),
           "env_state": t.backend.env.state(), "noise": t.rctx.rng_state(N.RNG_NOISE),
           "schedule": t.ctx.rng_state(N.RNG_SCHEDULE), "last_noise": t.noise.cpu().numpy()}
    for p in range(t.cfg.n_policies):
        out[f"adam{p}"] = list(t.ctx.adam_get(p))
    return out


@pytest.fixture(scope="module")
def solo_runs():
    """Two iterations of the solo trainer of every seed, one chain per fragment: (results, state)."""
    from ddrl_amd.trainer import PPOTrainer
    out = {}
    for s in SEEDS:
        tr = PPOTrainer(CONFIG, n_envs=8, seed=s)
        assert tr.fragment_chain
        results = [UNTIMED(tr.train()) for _ in range(2)]
        out[s] = (results, _trainer_state(tr))
        tr.stop()
    return out


@pytest.mark.parametrize("group_rollout", [None, False], ids=["group-rollout", "member-sampling"])
def test_population_members_equal_solo_trainers(solo_runs, group_rollout):
    from ddrl_amd.population import PopulationTrainer
    pop = PopulationTrainer(CONFIG, SEEDS, n_envs=8, group_rollout=group_rollout)
    assert pop.device_rng and (pop.rollout_group is not None) == (group_rollout is None)
    results = [pop.train() for _ in range(2)]
    for m, s in enumerate(SEEDS):
        for it in range(2):
            _same(UNTIMED(results[it][m]), solo_runs[s][0][it], f"seed {s} iteration {it}")
        _same(_trainer_state(pop.trainers[m]), solo_runs[s][1], f"seed {s} state")
    pop.stop()
    assert not np.array_equal(solo_runs[0][1]["last_noise"], solo_runs[1][1]["last_noise"])


def test_one_chain_fragment_equals_the_step_loop(solo_runs):
    from ddrl_amd.trainer import PPOTrainer
    tr = PPOTrainer(CONFIG, n_envs=8, seed=1)
    tr.fragment_chain = False   # act / env step / reward / observe call by call, reading slab[t]
    results = [UNTIMED(tr.train()) for _ in range(2)]
    _same(results, solo_runs[1][0], "results")
    _same(_trainer_state(tr), solo_runs[1][1], "state")
    tr.stop()


def test_the_default_backend_is_untouched_by_the_option(solo_runs):
    """rng_backend "host" spelled out is the default path (torch / numpy draws); the device backend
    is another stream of numbers."""
    from ddrl_amd.trainer import PPOTrainer
    host = {k: v for k, v in CONFIG.items() if k != "rng_backend"}
    a, b = PPOTrainer(host, n_envs=8, seed=1), PPOTrainer({**host, "rng_backend": "host"}, n_envs=8, seed=1)
    assert not hasattr(a, "noise") and a.rng_backend == b.rng_backend == "host"
    _same(UNTIMED(a.train()), UNTIMED(b.train()), "host results")
    _same(a.get_weights(), b.get_weights(), "host weights")
    assert not np.array_equal(list(a.get_weights().values())[0], list(solo_runs[1][1]["weights"].values())[0])
    a.stop(), b.stop()


def test_save_restore_continues_both_streams(tmp_path):
    import torch
    from ddrl_amd import native as N
    from ddrl_amd.trainer import PPOTrainer
    a = PPOTrainer(CONFIG, n_envs=8, seed=3)
    a.train()
    path = a.save(str(tmp_path / "ck.npz"))
    b = PPOTrainer(CONFIG, n_envs=8, seed=4)   # another seed: its own streams differ until the restore
    assert b.rctx.rng_state(N.RNG_NOISE) != a.rctx.rng_state(N.RNG_NOISE)
    b.restore(path)
    assert b.rctx.rng_state(N.RNG_NOISE) == a.rctx.rng_state(N.RNG_NOISE) == (4, 32)
    assert b.ctx.rng_state(N.RNG_SCHEDULE) == a.ctx.rng_state(N.RNG_SCHEDULE) == (3 + 7919, 1)
    for t in (a, b):
        t.rctx.noise_fill(t.T, t.noise)
        t._learn_schedules()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(b.noise.cpu().numpy(), a.noise.cpu().numpy())
    for p in range(4):
        np.testing.assert_array_equal(b.sched[0][p].cpu().numpy(), a.sched[0][p].cpu().numpy())
        np.testing.assert_array_equal(b.sched[1][p].cpu().numpy(), a.sched[1][p].cpu().numpy())
    # a file without the streams (written by a host-backend trainer) is accepted: the streams stay
    host = PPOTrainer({k: v for k, v in CONFIG.items() if k != "rng_backend"}, n_envs=8, seed=3)
    old = host.save(str(tmp_path / "host.npz"))
    before = (b.rctx.rng_state(N.RNG_NOISE), b.ctx.rng_state(N.RNG_SCHEDULE))
    b.restore(old)
    assert (b.rctx.rng_state(N.RNG_NOISE), b.ctx.rng_state(N.RNG_SCHEDULE)) == before
    for t in (a, b, host):
        t.stop()


def test_gather_mode_puts_each_stream_on_its_context():
    """parallel "gather": the noise stream on the rollout context, the schedule stream (the
    rank-independent seed) on the learner context of the union batch."""
    from ddrl_amd import native as N
    from ddrl_amd.trainer import PPOTrainer
    tr = PPOTrainer({**CONFIG, "parallel": "gather"}, n_envs=8, seed=2)
    assert tr.ctx is not tr.rctx
    assert tr.rctx.rng_state(N.RNG_NOISE) == (3, 0) and tr.ctx.rng_state(N.RNG_SCHEDULE) == (2 + 7919, 0)
    with pytest.raises(N.DdrlError, match="no seed"):
        tr.ctx.rng_state(N.RNG_NOISE)
    tr.train()
    assert tr.rctx.rng_state(N.RNG_NOISE) == (3, 32) and tr.ctx.rng_state(N.RNG_SCHEDULE) == (2 + 7919, 1)
    assert all(np.isfinite(w).all() for w in tr.get_weights().values())
    tr.stop()


def test_ddp_with_the_option_raises():
    from ddrl_amd.trainer import PPOTrainer
    with pytest.raises(ValueError, match="rng_backend 'device' does not cover parallel 'ddp'"):
        PPOTrainer({**CONFIG, "parallel": "ddp"}, n_envs=8)
    with pytest.raises(ValueError, match="rng_backend 'gpu'"):
        PPOTrainer({**CONFIG, "rng_backend": "gpu"}, n_envs=8)
