"""Batched policy evaluation on the device (ddrl_eval_*; eval.hip): the fused evaluation
forward against the rollout kernels (bit for bit) and the deterministic oracle, the episode
accounting against tests/eval_reference.py, state isolation from training, and the C++ loop over
the host env plane against the same steps issued one by one.

Reference: evaluation/rollout_episodes.py:26-164.  Tolerances: outputs that go through the fp32
forward use the rollout parity tolerance of tests/test_gpu_parity.py (1e-5 relative + 2e-5
absolute); the fp64 episode table uses 1e-12 (fp64 sums of a few hundred terms, the bound the
suite uses for the fp64 filter statistics)."""
import numpy as np
import pytest

from ddrl_amd import native as N
from ddrl_amd.spec import make_cfg
from oracle import ddrl_oracle as O
from tests import eval_reference as R
from tests.gpu_harness import (CUP_CONFIG, CUP_ENV, GNN_ENV, CupOracleRollout, OracleRollout, dev, init_params,
                               init_policy_params, run_rollout, synthetic_inputs)

pytestmark = pytest.mark.gpu
PARITY = dict(rtol=1e-5, atol=2e-5)


def _ctx(env, n, T, config=None, filter_update=1):
    import torch
    cfg, inst = make_cfg(env, n, T, config)
    cfg.filter_update = filter_update
    return N.Context(cfg, 0, torch.cuda.current_stream().cuda_stream), cfg, inst


def _filt(D, rng):
    return 100.0, rng.normal(size=D) * 0.1, np.abs(rng.normal(size=D)) * 99 + 1


def _logit_bufs(ctx, cfg):
    import torch
    return [torch.full((ctx.layout[p]["C"], 2 * cfg.act_dim), float("nan"), dtype=torch.float32, device="cuda")
            for p in range(cfg.n_policies)]


ACT_CASES = [
    pytest.param("QuantrupedMultiEnv_Local", 37, None, id="local37"),             # every 16-row tile ragged
    pytest.param("QuantrupedMultiEnv_Centralized", 70, None, id="centralized70"),   # A = 8, d = 43, two workgroups
    pytest.param("QuantrupedMultiEnv_TwoSides", 21, None, id="twosides21"),         # A = 4
    pytest.param("QuantrupedMultiEnv_SharedDecentral", 37, None, id="shared37"),    # k = 4: 148 rows
    pytest.param(CUP_ENV, 19, CUP_CONFIG, id="cup19"),                              # -1 / -2 constants, coupling
    pytest.param("QuantrupedMultiEnv_FullyDecentral", 37, {"env_config": {"target_velocity": [1.0]}}, id="tvel37"),
    pytest.param("QuantrupedMultiEnv_Local", 37, {"observation_filter": "MeanStdFilter"}, id="local37_pfilter"),
]


@pytest.mark.parametrize("env,n,config", ACT_CASES)
def test_eval_act_parity(env, n, config):
    """ddrl_eval_act against (a) ddrl_observe + ddrl_act of a twin context with filter_update = 0,
    bit for bit (actions and logits), (b) the deterministic oracle, (c) the env-side filter
    statistics of a twin that observes the same steps, bit for bit."""
    import torch
    T = 3
    cup = bool(config and (config.get("model") or {}).get("custom_model") == "cup")
    ectx, cfg, inst = _ctx(env, n, T, config)
    twin0, _, _ = _ctx(env, n, T, config, filter_update=0)
    twin1, _, _ = _ctx(env, n, T, config, filter_update=1)
    rng = np.random.default_rng(31)
    params = init_policy_params(ectx, cfg, 5, cup)
    for c in (twin0, twin1):
        init_policy_params(c, cfg, 5, cup)
    D, A = cfg.obs_full_dim, cfg.act_dim
    assert D == (44 if "target_velocity" in str(config) else 43)
    filt = _filt(D, rng)
    obs, eps, _, _, _ = synthetic_inputs(rng, cfg, T)
    orc = (CupOracleRollout if cup else OracleRollout)(cfg, inst, params, filt)
    pfilt = None
    if cfg.policy_filter:
        pfilt = [(500.0, rng.normal(size=cfg.obs_dim[p]) * 0.2, np.abs(rng.normal(size=cfg.obs_dim[p])) * 499 + 5)
                 for p in range(cfg.n_policies)]
    for c in (ectx, twin0, twin1):
        c.filter_set(*filt)
        for p in range(cfg.n_policies if pfilt else 0):
            c.policy_filter_set(p, *pfilt[p])

    act_t = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    act_e = torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda")
    act_d = torch.full((n, 8), float("nan"), dtype=torch.float32, device="cuda")
    ectx.eval_begin(1, filter_update=False)
    inside = total = 0
    for t in range(T):
        o_t, e_t = dev(obs[t]), dev(eps[t])
        twin0.observe(o_t)
        twin0.act(t, e_t, act_t)
        twin0.synchronize()
        pstate = None
        if pfilt:   # the twin's observe pushed into its per-policy filters: evaluate with the same state
            pstate = [twin0.policy_filter_get(p) for p in range(cfg.n_policies)]
            for p in range(cfg.n_policies):
                ectx.policy_filter_set(p, *pstate[p])
                orc.pf[p].n, orc.pf[p].M[:], orc.pf[p].S[:] = pstate[p]
        # (a) with noise: bit-identical to observe + act
        lg_e, lg_d = _logit_bufs(ectx, cfg), _logit_bufs(ectx, cfg)
        ectx.eval_act(o_t, e_t, act_e, lg_e)
        ectx.eval_act(o_t, None, act_d, lg_d)
        ectx.synchronize()
        np.testing.assert_array_equal(act_e.cpu().numpy(), act_t.cpu().numpy(), err_msg=f"step {t} actions")
        for p in range(cfg.n_policies):
            lay = ectx.layout[p]
            C = lay["C"]
            rec = twin0.records_get(p)[t * C:(t + 1) * C, lay["logit"]:lay["logit"] + 2 * A]
            np.testing.assert_array_equal(lg_e[p].cpu().numpy(), rec, err_msg=f"step {t} p{p} logits")
            np.testing.assert_array_equal(lg_d[p].cpu().numpy(), rec, err_msg=f"step {t} p{p} logits (no noise)")
        # (b) deterministic: the oracle's clip(mean)
        R.eval_observe(orc, obs[t], filter_update=False)
        a_orc, lg_orc = R.eval_act(orc, None)
        a_det = act_d.cpu().numpy()
        np.testing.assert_allclose(a_det, a_orc, err_msg=f"step {t} deterministic actions", **PARITY)
        for p in range(cfg.n_policies):
            np.testing.assert_allclose(lg_d[p].cpu().numpy(), lg_orc[p], err_msg=f"step {t} p{p}", **PARITY)
        inside += int((np.abs(a_det) < 1.0).sum())
        total += a_det.size
        # (c) filter_update = 0: nothing moves
        fn, fM, fS = ectx.filter_get()
        assert fn == filt[0] and np.array_equal(fM, filt[1]) and np.array_equal(fS, filt[2])
        if pfilt:
            for p in range(cfg.n_policies):
                got = ectx.policy_filter_get(p)
                assert got[0] == pstate[p][0] and np.array_equal(got[1], pstate[p][1]) and np.array_equal(got[2], pstate[p][2])
    assert inside * 2 >= total, (inside, total)   # a good share of the means is unclipped
    ectx.eval_end()

    # (c) filter_update = 1: the env-side statistics follow a twin's observe calls bit for bit
    ectx.eval_begin(1, filter_update=True)
    pbefore = [ectx.policy_filter_get(p) for p in range(cfg.n_policies)]
    for t in range(T):
        o_t = dev(obs[t])
        ectx.eval_act(o_t, None, act_d)
        twin1.observe(o_t)
    ectx.synchronize()
    twin1.synchronize()
    got, want = ectx.filter_get(), twin1.filter_get()
    assert got[0] == want[0] == filt[0] + T * n
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    dgot, dwant = ectx.filter_delta_get(), twin1.filter_delta_get()
    assert dgot[0] == dwant[0] and np.array_equal(dgot[1], dwant[1]) and np.array_equal(dgot[2], dwant[2])
    for p in range(cfg.n_policies):
        after = ectx.policy_filter_get(p)
        assert after[0] == pbefore[p][0] and np.array_equal(after[1], pbefore[p][1]) and np.array_equal(after[2], pbefore[p][2])
    ectx.eval_end()
    for c in (ectx, twin0, twin1):
        c.close()


# ---- episode accounting ---------------------------------------------------------------
def _scripted(cfg, T, n, seed=43):
    rng = np.random.default_rng(seed)
    _, _, fw, cfrc, _ = synthetic_inputs(rng, cfg, T)
    actions = rng.uniform(-1.0, 1.0, size=(T, n, 8)).astype(np.float32)
    kin = rng.normal(size=(T, n, 9)).astype(np.float32)
    return fw, cfrc, actions, kin, R.scripted_done(T, n)


def _run_scripted(ctx, cfg, inst, E, inputs, filter_update=False):
    fw, cfrc, actions, kin, done = inputs
    T, n = done.shape
    ref = R.EpisodeAccumulator(n, E)
    ctx.eval_begin(E, filter_update=filter_update)
    for t in range(T):
        ctx.eval_step(dev(fw[t]), dev(cfrc[t]), dev(actions[t]), dev(kin[t]), dev(done[t]))
        ref.step(R.step_rewards(cfg, inst, fw[t], cfrc[t], actions[t]), actions[t], kin[t], done[t])
    progress = ctx.eval_progress()
    table = ctx.eval_results()
    ctx.eval_end()
    return table, progress, ref


def test_scripted_done_pattern_covers_every_class():
    """Guards the input of the accounting tests: the seeded 12 x 37 pattern has envs that never
    fill a quota of 2 (some without any episode), envs with exactly 2 ends, with more, envs
    stepped after their quota, and one-step episodes."""
    done = np.random.default_rng(41).random((12, 37)) < 0.25
    cnt = done.sum(0)
    last_quota = np.array([np.flatnonzero(done[:, e])[1] if cnt[e] >= 2 else 99 for e in range(37)])
    one_step = sum(int(done[0, e]) + int((done[1:, e] & done[:-1, e]).sum()) for e in range(37))
    classes = dict(never_fill=int((cnt < 2).sum()), no_episode=int((cnt == 0).sum()), exactly_two=int((cnt == 2).sum()),
                   more=int((cnt > 2).sum()), stepped_after_quota=int((last_quota < 11).sum()), one_step=one_step)
    assert all(v >= 3 for k, v in classes.items() if k != "no_episode") and classes["no_episode"] >= 1, classes


@pytest.mark.parametrize("n,config", [pytest.param(37, None, id="per_leg37"),
                                      pytest.param(19, {"env_config": {"global_reward": True}}, id="global19"),
                                      pytest.param(19, {"env_config": {"norm_reward": True}}, id="norm19")])
def test_episode_accounting_scripted(n, config):
    _episode_accounting(n, config, 37)


@pytest.mark.parametrize("n,config", [pytest.param(64, None, id="per_leg64"),      # one exactly full block
                                      pytest.param(70, None, id="per_leg70"),      # two blocks, clamped tail lanes
                                      pytest.param(64, {"env_config": {"global_reward": True}}, id="global64"),
                                      pytest.param(70, {"env_config": {"norm_reward": True}}, id="norm70")])
def test_episode_accounting_multi_block(n, config):
    """k_eval_accum over more than its first block (64 envs x 4 lanes): inputs generated at n, whose
    done pattern tests/test_rollout_edge_inputs.py guards."""
    _episode_accounting(n, config, n)


def _episode_accounting(n, config, n_inputs):
    ctx, cfg, inst = _ctx("QuantrupedMultiEnv_Local", n, 4, config)
    mode = {None: N.REWARD_PER_LEG, "global_reward": N.REWARD_GLOBAL, "norm_reward": N.REWARD_NORM}[
        next(iter(config["env_config"])) if config else None]
    assert cfg.reward_mode == mode
    E, T = 2, 12
    inputs = _scripted(cfg, T, n_inputs)
    inputs = tuple(a[:, :n] for a in inputs)
    table, progress, ref = _run_scripted(ctx, cfg, inst, E, inputs)
    assert table.shape == (n, E, 6) and table.dtype == np.float64
    np.testing.assert_array_equal(np.isnan(table), np.isnan(ref.table))   # NaN rows: exactly the unfilled ones
    filled = ~np.isnan(ref.table[:, :, 0])
    assert np.array_equal(np.isnan(table).all(2), ~filled) and np.array_equal(np.isnan(table).any(2), ~filled)
    np.testing.assert_allclose(table, ref.table, rtol=1e-12, atol=1e-12, equal_nan=True)
    np.testing.assert_array_equal(table[filled][:, 1], ref.table[filled][:, 1])   # durations exact
    assert progress == (ref.episodes_done, ref.envs_finished) == (int(filled.sum()), int(filled.all(1).sum()))
    assert 0 < ref.envs_finished < n
    # a second begin clears everything
    ctx.eval_begin(E)
    assert ctx.eval_progress() == (0, 0) and np.isnan(ctx.eval_results()).all()
    ctx.eval_end()
    ctx.close()


REWARD_MODES = [pytest.param(None, N.REWARD_PER_LEG, id="per_leg"),
                pytest.param({"env_config": {"global_reward": True}}, N.REWARD_GLOBAL, id="global"),
                pytest.param({"env_config": {"norm_reward": True}}, N.REWARD_NORM, id="norm")]


@pytest.mark.parametrize("config,mode", REWARD_MODES)
@pytest.mark.parametrize("env,n", [
    pytest.param("QuantrupedMultiEnv_Local", 5, id="local5"),       # a ragged last group of four lanes
    pytest.param("QuantrupedMultiEnv_Local", 65, id="local65"),     # the second 256-thread block
    pytest.param("QuantrupedMultiEnv_SharedDecentral", 5, id="shared5")])   # k = 4: one policy, four slots
def test_reward_record_and_episode_return_agree(env, n, config, mode):
    """The two consumers of the per-agent reward on the same context and inputs: ddrl_reward rounds
    every agent's fp64 reward to fp32 into its record, ddrl_eval_step sums the same fp64 rewards.
    With every env done at its first step the table's return is that sum, so it differs from the
    fp64 sum of the env's record fields r_j by the records' roundings alone: at most
    sum_j |r_j| 2^-24 (half an ulp each), with 1e-9 of slack for the fp64 additions."""
    ctx, cfg, inst = _ctx(env, n, 1, config)
    assert cfg.reward_mode == mode
    fw, cfrc, actions, kin, _ = _scripted(cfg, 1, n)
    f_d, c_d, a_d = dev(fw[0]), dev(cfrc[0]), dev(actions[0])
    ctx.reward(0, f_d, c_d, a_d)
    ctx.eval_begin(1)
    ctx.eval_step(f_d, c_d, a_d, dev(kin[0]), dev(np.ones(n, np.uint8)))
    ret = ctx.eval_results()[:, 0, 0]
    ctx.eval_end()
    r = np.zeros((n, cfg.n_agents))   # the fp32 record fields, exact in fp64
    for p in range(cfg.n_policies):
        agents = [j for j in range(cfg.n_agents) if cfg.agent_policy[j] == p]
        lay = ctx.layout[p]
        rew = ctx.records_get(p)[:lay["C"], lay["rew"]].reshape(n, len(agents))
        assert rew.dtype == np.float32
        for slot, j in enumerate(agents):
            r[:, j] = rew[:, slot]
    ctx.close()
    assert np.isfinite(ret).all() and (r != 0).all()
    total = np.zeros(n)
    for j in range(cfg.n_agents):   # agent order, as the accumulator adds
        total += r[:, j]
    err, bound = np.abs(ret - total), np.abs(r).sum(1) * 2.0 ** -24 * (1 + 1e-9)
    print(f"max |return - sum of records| = {err.max():.3e}, largest share of its bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), (err / bound).max()
    assert (err > 0).any()   # the return is not the sum of the rounded records


def test_zero_distance_episode_gives_ieee_results():
    ctx, cfg, inst = _ctx("QuantrupedMultiEnv_Local", 3, 2)
    z = lambda *s: np.zeros(s, np.float32)
    kin = z(3, 9)
    kin[:, 1:] = 1.0
    kin[1, 0] = 0.5
    act = z(3, 8)
    act[:2] = 0.5         # env 2: no power either -> 0 / 0
    ctx.eval_begin(1)
    ctx.eval_step(dev(z(3)), dev(z(3, 14, 6)), dev(act), dev(kin), dev(np.ones(3, np.uint8)))
    t = ctx.eval_results()[:, 0]
    assert t[0, 2] == 0 and t[0, 4] == 0 and np.isposinf(t[0, 5])          # distance 0: velocity 0, CoT inf
    assert t[1, 4] == 0.5 and t[1, 5] == (4.0 / 1) / (N.TOTAL_MASS * 0.5)  # 8 joints x |0.5 * 1|
    assert t[2, 3] == 0 and np.isnan(t[2, 5]) and t[2, 1] == 1
    ctx.eval_end()
    ctx.close()


def test_evaluation_leaves_the_training_state_alone():
    """On a context that holds a finished rollout, an evaluation (forward + accounting, filter
    frozen) changes nothing the training path reads, and the update that follows gives the
    parameters of a twin context that never evaluated, bit for bit."""
    import torch
    n, T = 37, 4
    ctxs = []
    for _ in range(2):
        ctx, cfg, inst = _ctx("QuantrupedMultiEnv_Local", n, T)
        params = init_params(ctx, cfg, 3, head_scale=1.0)
        rng = np.random.default_rng(13)
        run_rollout(ctx, cfg, inst, params, rng, _filt(43, rng), T)
        ctxs.append(ctx)
    ctx, twin = ctxs
    P = cfg.n_policies

    def state(c):
        c.synchronize()
        out = [np.asarray(c.filter_get()[0])] + list(c.filter_get()[1:])
        for p in range(P):
            m, v, b1, b2 = c.adam_get(p)
            pf = c.policy_filter_get(p)
            out += [c.records_get(p), c.params_get(p), m, v, np.array([b1, b2]), c.last_values_get(p),
                    c.adv_norm_get(p), np.asarray(pf[0]), pf[1], pf[2]]
        return out

    before = state(ctx)
    inputs = _scripted(cfg, 12, n)
    obs = synthetic_inputs(np.random.default_rng(2), cfg, 12)[0]
    eps = synthetic_inputs(np.random.default_rng(2), cfg, 12)[1]
    actions = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    ctx.eval_begin(2, filter_update=False)
    for t in range(12):
        ctx.eval_act(dev(obs[t]), dev(eps[t]) if t % 2 else None, actions)
        ctx.eval_step(dev(inputs[0][t]), dev(inputs[1][t]), actions, dev(inputs[3][t]), dev(inputs[4][t]))
    assert ctx.eval_progress()[0] > 0
    ctx.eval_end()
    for a, b in zip(before, state(ctx)):
        np.testing.assert_array_equal(a, b)
    rs = np.random.default_rng(8)
    sched = [O.sgd_schedule(rs, T * ctx.layout[p]["C"], 128, cfg.num_sgd_iter) for p in range(P)]
    for c in (ctx, twin):
        c.gae()
        c.ppo_update((1 << P) - 1, [dev(s[0]) for s in sched], [dev(s[1]) for s in sched], [0.2] * P, max_steps=2)
        c.synchronize()
    for p in range(P):
        assert not np.array_equal(ctx.params_get(p), before[3 + 10 * p + 1])   # the update moved them
        np.testing.assert_array_equal(ctx.params_get(p), twin.params_get(p))
    ctx.close()
    twin.close()


@pytest.mark.parametrize("explore", [False, True], ids=["deterministic", "noise"])
def test_hostenv_loop_matches_stepwise(explore):
    """ddrl_eval_hostenv (loop in C++) against eval_act / host step / eval_step issued one by one,
    fully synchronized, on a twin context and env plane with the same seed."""
    import torch
    n, E, limit, poll, max_steps = 24, 2, 40, 5, 100
    rng = np.random.default_rng(6)
    filt = _filt(43, rng)
    eps = torch.from_numpy(rng.normal(size=(max_steps, n, 4, 2)).astype(np.float32)).cuda() if explore else None
    pair = []
    for _ in range(2):
        ctx, cfg, inst = _ctx("QuantrupedMultiEnv_Local", n, 1)
        init_params(ctx, cfg, 9, head_scale=1.0)
        ctx.filter_set(*filt)
        env = N.HostEnv(n, 43, n_threads=2, seed=21)
        env.set_time_limit(limit)
        ctx.eval_begin(E, filter_update=True)
        pair.append((ctx, env))
    (ca, ea), (cb, eb) = pair
    steps_a = ca.eval_hostenv(ea, eps, max_steps if explore else 0, max_steps, poll_every=poll)

    actions = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    obs = eb.reset_episodes()
    dsum, host_dist, steps_b = np.zeros(n), [[] for _ in range(n)], 0
    while steps_b < max_steps:
        cb.eval_act(dev(obs), eps[steps_b] if explore else None, actions)
        cb.synchronize()
        eb.act[:] = actions.cpu().numpy()
        eb.step()
        dsum += eb.kin[:, 0].astype(np.float64)
        for e in np.flatnonzero(eb.done):
            host_dist[e].append(dsum[e])
            dsum[e] = 0.0
        cb.eval_step(dev(eb.fw.copy()), dev(eb.cfrc.copy()), actions, dev(eb.kin.copy()), dev(eb.done.copy()))
        cb.synchronize()
        obs = eb.obs.copy()
        steps_b += 1
        if steps_b % poll == 0 and cb.eval_progress()[1] == n:
            break
    assert steps_a == steps_b and 1 < steps_a <= E * limit
    ta, tb = ca.eval_results(), cb.eval_results()
    np.testing.assert_array_equal(ta, tb)
    assert not np.isnan(ta).any() and ca.eval_progress() == (n * E, n)
    for x, y in zip(ca.filter_get(), cb.filter_get()):
        np.testing.assert_array_equal(x, y)
    assert ca.filter_get()[0] == filt[0] + steps_a * n
    assert ta[:, :, 1].max() <= limit and ta[:, :, 1].min() >= 1
    want = np.array([host_dist[e][:E] for e in range(n)])
    np.testing.assert_allclose(ta[:, :, 2], want, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(ta[:, :, 4], ta[:, :, 2] / ta[:, :, 1])
    for c, e in pair:
        c.eval_end()
        c.close()
        e.close()


def test_graphnet_contexts_are_refused():
    ctx, cfg, inst = _ctx(GNN_ENV, 8, 2)
    with pytest.raises(N.DdrlError, match="fcnet"):
        ctx.eval_begin(1)
    ctx.close()


def test_unbegun_and_null_calls_fail_with_messages():
    import torch
    ctx, cfg, inst = _ctx("QuantrupedMultiEnv_Local", 4, 2)
    buf = torch.zeros(4 * 14 * 6, dtype=torch.float32, device="cuda")
    env = N.HostEnv(4, 43)
    for call in (lambda: ctx.eval_act(buf, None, buf), lambda: ctx.eval_step(buf, buf, buf, buf, buf),
                 ctx.eval_progress, ctx.eval_end, lambda: ctx.eval_hostenv(env),
                 lambda: N._ck(ctx.lib.ddrl_eval_results(ctx.h, buf.data_ptr(), 4))):
        with pytest.raises(N.DdrlError, match="ddrl_eval_begin first"):
            call()
    with pytest.raises(N.DdrlError, match="episodes_per_env"):
        ctx.eval_begin(0)
    with pytest.raises(N.DdrlError, match="null evaluation config"):
        N._ck(ctx.lib.ddrl_eval_begin(ctx.h, None))
    ctx.eval_begin(1)
    with pytest.raises(N.DdrlError, match="null"):
        ctx.eval_act(None, None, buf)
    with pytest.raises(N.DdrlError, match="null"):
        ctx.eval_act(buf, None, None)
    with pytest.raises(N.DdrlError, match="null"):
        ctx.eval_step(buf, buf, buf, None, buf)
    with pytest.raises(N.DdrlError, match="null"):
        ctx.eval_step(buf, buf, buf, buf, None)
    with pytest.raises(N.DdrlError, match="rows"):
        N._ck(ctx.lib.ddrl_eval_results(ctx.h, buf.data_ptr(), 3))
    with pytest.raises(N.DdrlError, match="shape"):
        env5 = N.HostEnv(5, 43)
        try:
            ctx.eval_hostenv(env5)
        finally:
            env5.close()
    with pytest.raises(N.DdrlError, match="max_steps"):
        ctx.eval_hostenv(env, max_steps=0)
    ctx.eval_end()
    env.close()
    ctx.close()
