"""Input sensitivity of the evaluated policies on the device (ddrl_eval_sens_*; eval_sens.hip):
the perturbed rows against the existing evaluation kernel bit for bit, the fp64 accumulation, the
oracle restatement of tests/sens_reference.py, the episode-quota gate, isolation from training and
from the evaluation itself, and the refusals.

Reference: evaluation/rollout_episodes_compute_gradient.py:59-68, :111-122, :167-168.
Tolerances: a clipped mean goes through the fp32 forward, so it carries the rollout parity
tolerance of tests/test_gpu_parity.py (1e-5 |m| + 2e-5 <= 3e-5 for |m| <= 1); a difference of
two carries twice that plus the rounding of one fp32 subtraction (< 1.2e-7), so a sum of `rows`
differences is within rows * 6.1e-5 of the reference.  fp64 sums use 1e-12 * sum |terms|, the
bound the suite uses for fp64 sums."""
import functools

import numpy as np
import pytest

from ddrl_amd import native as N
from ddrl_amd.spec import make_cfg
from oracle import ddrl_oracle as O
from tests import eval_reference as R
from tests import sens_reference as S
from tests.gpu_harness import (GNN_ENV, OracleRollout, dev, init_params, init_policy_params, run_rollout,
                               synthetic_inputs)

pytestmark = pytest.mark.gpu
PARITY = dict(rtol=1e-5, atol=2e-5)
T, CASES, ORACLE_CASES = S.T, S.CASES, S.ORACLE_CASES
TVEL, PFILTER = S.TVEL, S.PFILTER
# bit identity also with the per-policy filter switched the other way
GRID_CASES = dict(CASES, central_tvel3_pfilter=("QuantrupedMultiEnv_Centralized", 3, {**TVEL, **PFILTER}, None),
                  local5=("QuantrupedMultiEnv_Local", 5, None, None))


def _merge(config, env_config):
    config = dict(config or {})
    config["env_config"] = {**config.get("env_config", {}), **env_config}
    return config


def _ctx(env, n, config=None, frag=T):
    import torch
    cfg, inst = make_cfg(env, n, frag, config)
    return N.Context(cfg, 0, torch.cuda.current_stream().cuda_stream), cfg, inst


def _means_bufs(ctx, cfg):
    import torch
    return [torch.full((ctx.layout[p]["C"], 2 * cfg.obs_dim[p], cfg.act_dim), 7.0, dtype=torch.float32, device="cuda")
            for p in range(cfg.n_policies)]


def _slots(cfg):
    return [[j for j in range(cfg.n_agents) if cfg.agent_policy[j] == p] for p in range(cfg.n_policies)]


def grid_inputs(cfg, seed=17):
    """Observations [T, n, D] and steps on a 2^-10 grid, |x| < 8, 0 < h <= 0.25: x +- h is exact in
    fp32 and fp64."""
    rng = np.random.default_rng(seed)
    obs = (rng.integers(-8 * 1024 + 1, 8 * 1024, size=(T, cfg.n_envs, cfg.obs_full_dim)) / 1024.0).astype(np.float32)
    steps = [rng.integers(1, 257, size=cfg.obs_dim[p]) / 1024.0 for p in range(cfg.n_policies)]
    return obs, steps


@functools.lru_cache(maxsize=None)
def _grid_run(name, compare_act):
    """One evaluation of T steps on the grid inputs with the env-side filter off.  Returns
    (cfg, means per step and policy, results per policy, mismatches of the eval_act comparison)."""
    import os
    import torch
    env, n, config, grid = GRID_CASES[name]
    config = _merge(config, {"observation_filter_env": False})
    ctx, cfg, inst = _ctx(env, n, config)
    old = os.environ.pop("DDRL_SENS_GRID", None)
    if grid:
        os.environ["DDRL_SENS_GRID"] = str(grid)
    try:
        init_policy_params(ctx, cfg, 5, S.is_cup(config))
        rng = np.random.default_rng(3)
        if cfg.policy_filter:
            for p, st in enumerate(S.pfilt(cfg, rng)):
                ctx.policy_filter_set(p, *st)
        obs, steps = grid_inputs(cfg)
        A = cfg.act_dim
        act = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
        ctx.eval_begin(1, filter_update=False)
        ctx.eval_sens_begin(steps)
        means, bad = [], []
        for t in range(T):
            o_t = dev(obs[t])
            bufs = _means_bufs(ctx, cfg)
            ctx.eval_act(o_t, None, act)
            ctx.eval_sens(o_t, bufs)
            ctx.synchronize()
            got = [b.cpu().numpy() for b in bufs]
            means.append(got)
            if not compare_act:
                continue
            # every (policy, slot, feature, sign): ddrl_eval_act on the observation with that one
            # column moved; only the rows whose feature the column is are compared
            jobs, outs = [], []
            for p, agents in enumerate(_slots(cfg)):
                k, d = len(agents), cfg.obs_dim[p]
                for s, j in enumerate(agents):
                    cols = [cfg.obs_index[j][f] for f in range(d)]
                    real = [c for c in cols if c >= 0]
                    assert len(set(real)) == len(real)   # a column is one feature of a row at most
                    for f, col in enumerate(cols):
                        if col < 0:
                            assert np.isnan(got[p][s::k, 2 * f:2 * f + 2]).all(), (name, p, s, f)
                            continue
                        for sign in (0, 1):
                            moved = obs[t].copy()
                            moved[:, col] += np.float32(steps[p][f] if sign else -steps[p][f])
                            assert np.all(moved[:, col].astype(np.float64) ==
                                          obs[t][:, col].astype(np.float64) + (steps[p][f] if sign else -steps[p][f]))
                            lg = torch.full((ctx.layout[p]["C"], 2 * A), float("nan"), dtype=torch.float32, device="cuda")
                            ctx.eval_act(dev(moved), None, act, [lg if q == p else None for q in range(cfg.n_policies)])
                            jobs.append((p, s, k, f, sign))
                            outs.append(lg)
            ctx.synchronize()
            for (p, s, k, f, sign), lg in zip(jobs, outs):
                want = np.clip(lg.cpu().numpy()[s::k, :A], -1.0, 1.0)   # logits_out carries the coupling already
                if not np.array_equal(got[p][s::k, 2 * f + sign], want):
                    bad.append((t, p, s, f, sign, float(np.abs(got[p][s::k, 2 * f + sign] - want).max())))
        res = [ctx.eval_sens_results(p) for p in range(cfg.n_policies)]
        ctx.eval_end()
    finally:
        os.environ.pop("DDRL_SENS_GRID", None)
        if old is not None:
            os.environ["DDRL_SENS_GRID"] = old
        ctx.close()
    return cfg, means, res, bad


@pytest.mark.parametrize("name", list(GRID_CASES))
def test_perturbed_rows_equal_eval_act_bit_for_bit(name):
    """means_out of row 2f / 2f + 1 == clip(mean of ddrl_eval_act) on the observation whose column
    obs_index[slot][f] is moved by -h_f / +h_f, for every feature, sign, slot and policy."""
    cfg, means, res, bad = _grid_run(name, True)
    if name == "central_tvel3":
        assert cfg.obs_dim[0] == 44 and cfg.act_dim == 8
    if name == "legid3":
        assert cfg.obs_dim[0] == 23 and sum(cfg.obs_index[0][f] < 0 for f in range(23)) == 4
    assert not bad, bad[:5]
    for t in range(T):
        for p in range(cfg.n_policies):
            assert not (means[t][p] == 7.0).any()                       # every row was written
            assert (np.abs(means[t][p][~np.isnan(means[t][p])]) <= 1.0).all()


@pytest.mark.parametrize("name", list(GRID_CASES))
def test_accumulation_is_the_fp64_sum_and_deterministic(name):
    cfg, means, res, _ = _grid_run(name, True)
    _, means2, res2, _ = _grid_run(name, False)   # a second context, the same calls
    for p in range(cfg.n_policies):
        terms = np.concatenate([S.terms(means[t][p]) for t in range(T)]).astype(np.float64)   # [T C, d, A]
        grads, grads_abs, rows = res[p]
        mag = np.abs(terms).sum(0)
        assert rows == terms.shape[0] == T * cfg.n_envs * len(_slots(cfg)[p])
        assert (np.abs(grads - terms.sum(0)) <= 1e-12 * mag).all()
        assert (np.abs(grads_abs - mag) <= 1e-12 * mag).all()
        assert mag.max() > 0
        for a, b in zip(res[p], res2[p]):
            np.testing.assert_array_equal(a, b)
        for t in range(T):
            np.testing.assert_array_equal(means[t][p], means2[t][p])


# ---- oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_matrices_match_the_oracle(name):
    import os
    import torch
    env, n, config, grid = ORACLE_CASES[name]
    _, inst, config, filt, pfilt, obs, steps = S.oracle_case(name)
    ctx, cfg, _ = _ctx(env, n, config)
    params = init_policy_params(ctx, cfg, 5, S.is_cup(config))
    orc = S.make_oracle(cfg, inst, config, params, filt, pfilt)
    ctx.filter_set(*filt)
    for p, st in enumerate(pfilt or []):
        ctx.policy_filter_set(p, *st)
    act = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    ref = S.SensAccumulator(cfg)
    old = os.environ.pop("DDRL_SENS_GRID", None)
    if grid:
        os.environ["DDRL_SENS_GRID"] = str(grid)
    try:
        ctx.eval_begin(1, filter_update=False)
        ctx.eval_sens_begin(steps)
        inside = total = 0
        for t in range(T):
            o_t = dev(obs[t])
            bufs = _means_bufs(ctx, cfg)
            ctx.eval_act(o_t, None, act)
            ctx.eval_sens(o_t, bufs)
            want = S.sens_means(orc, obs[t], steps)
            ref.step([w[0] for w in want])
            for p in range(cfg.n_policies):
                np.testing.assert_allclose(bufs[p].cpu().numpy(), want[p][0], err_msg=f"step {t} p{p}", **PARITY)
                inside += int((np.abs(want[p][1]) < 1.0).sum())
                total += want[p][1].size
        assert inside * 2 >= total, (inside, total)
        for p in range(cfg.n_policies):
            grads, grads_abs, rows = ctx.eval_sens_results(p)
            moved = want[p][2]                                   # [k, d]
            assert rows == ref.rows[p] == T * cfg.n_envs * moved.shape[0]
            print(name, p, "max |grads - ref|", np.abs(grads - ref.grads[p]).max(), "bound", rows * 6.1e-5)
            assert (np.abs(grads - ref.grads[p]) <= rows * 6.1e-5).all()
            assert (np.abs(grads_abs - ref.grads_abs[p]) <= rows * 6.1e-5).all()
            const = ~moved.any(0)
            assert (grads[const] == 0).all() and (grads_abs[const] == 0).all()
            assert (grads_abs[~const] != 0).mean() >= 0.9
        ctx.eval_end()
    finally:
        os.environ.pop("DDRL_SENS_GRID", None)
        if old is not None:
            os.environ["DDRL_SENS_GRID"] = old
        ctx.close()


# ---- quota gate -----------------------------------------------------------------------------
def test_quota_gate_follows_the_episode_table():
    """Stepwise eval_act -> eval_sens -> eval_step over the scripted done pattern with E = 2: an env
    contributes at a step exactly while count[e] < E before that step's eval_step."""
    import torch
    n, E, steps_n = 37, 2, 12
    ctx, cfg, inst = _ctx("QuantrupedMultiEnv_Local", n, None, frag=4)
    params = init_policy_params(ctx, cfg, 9, False)
    rng = np.random.default_rng(43)
    filt = S.filt(cfg.obs_full_dim, rng)
    obs, _, fw, cfrc, _ = synthetic_inputs(rng, cfg, steps_n)
    actions = rng.uniform(-1.0, 1.0, size=(steps_n, n, 8)).astype(np.float32)
    kin = rng.normal(size=(steps_n, n, 9)).astype(np.float32)
    done = R.scripted_done(steps_n, n)
    classes = R.done_classes(done, E)
    assert classes["never_fill"] >= 3 and classes["stepped_after_quota"] >= 3, classes
    orc = OracleRollout(cfg, inst, params, filt)
    ctx.filter_set(*filt)
    hs = [np.full(cfg.obs_dim[p], 0.1) for p in range(cfg.n_policies)]
    act = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    acc, ref, own = R.EpisodeAccumulator(n, E), S.SensAccumulator(cfg), S.SensAccumulator(cfg)
    ctx.eval_begin(E, filter_update=False)
    ctx.eval_sens_begin(hs)
    for t in range(steps_n):
        o_t = dev(obs[t])
        bufs = _means_bufs(ctx, cfg)
        ctx.eval_act(o_t, None, act)
        ctx.eval_sens(o_t, bufs)
        ctx.eval_step(dev(fw[t]), dev(cfrc[t]), dev(actions[t]), dev(kin[t]), dev(done[t]))
        env_open = np.array(acc.count) < E
        ref.step([w[0] for w in S.sens_means(orc, obs[t], hs)], env_open)
        own.step([b.cpu().numpy() for b in bufs], env_open)
        acc.step(R.step_rewards(cfg, inst, fw[t], cfrc[t], actions[t]), actions[t], kin[t], done[t])
    assert 0 < ref.rows[0] < steps_n * n
    for p in range(cfg.n_policies):
        grads, grads_abs, rows = ctx.eval_sens_results(p)
        assert rows == ref.rows[p]
        assert (np.abs(grads - own.grads[p]) <= 1e-12 * own.mag[p]).all()        # exactly the gated terms
        assert (np.abs(grads_abs - own.grads_abs[p]) <= 1e-12 * own.mag[p]).all()
        assert (np.abs(grads - ref.grads[p]) <= rows * 6.1e-5).all()
        assert (np.abs(grads_abs - ref.grads_abs[p]) <= rows * 6.1e-5).all()
    assert ctx.eval_progress() == (acc.episodes_done, acc.envs_finished)
    ctx.eval_end()
    ctx.close()


# ---- isolation ------------------------------------------------------------------------------
def test_sensitivity_leaves_the_training_state_alone():
    """test_evaluation_leaves_the_training_state_alone (tests/test_gpu_eval.py) with the sensitivity
    calls in the evaluation: the training state, the filters and the update that follows are those
    of a twin that never ran them, bit for bit."""
    import torch
    n, frag = 37, 4
    ctxs = []
    for _ in range(2):
        ctx, cfg, inst = _ctx("QuantrupedMultiEnv_Local", n, None, frag=frag)
        params = init_params(ctx, cfg, 3, head_scale=1.0)
        rng = np.random.default_rng(13)
        run_rollout(ctx, cfg, inst, params, rng, S.filt(43, rng), frag)
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
    rng = np.random.default_rng(2)
    obs, _, fw, cfrc, _ = synthetic_inputs(rng, cfg, 6)
    kin = rng.normal(size=(6, n, 9)).astype(np.float32)
    done = R.scripted_done(6, n)
    actions = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    ctx.eval_begin(2, filter_update=False)
    ctx.eval_sens_begin([np.full(cfg.obs_dim[p], 0.1) for p in range(P)])
    for t in range(6):
        ctx.eval_act(dev(obs[t]), None, actions)
        ctx.eval_sens(dev(obs[t]), _means_bufs(ctx, cfg) if t % 2 else None)
        ctx.eval_step(dev(fw[t]), dev(cfrc[t]), actions, dev(kin[t]), dev(done[t]))
    assert ctx.eval_sens_results(0)[2] > 0
    ctx.eval_end()
    for a, b in zip(before, state(ctx)):
        np.testing.assert_array_equal(a, b)
    rs = np.random.default_rng(8)
    sched = [O.sgd_schedule(rs, frag * ctx.layout[p]["C"], 128, cfg.num_sgd_iter) for p in range(P)]
    for c in (ctx, twin):
        c.gae()
        c.ppo_update((1 << P) - 1, [dev(s[0]) for s in sched], [dev(s[1]) for s in sched], [0.2] * P, max_steps=2)
        c.synchronize()
    for p in range(P):
        assert not np.array_equal(ctx.params_get(p), before[3 + 10 * p + 1])   # the update moved them
        np.testing.assert_array_equal(ctx.params_get(p), twin.params_get(p))
    ctx.close()
    twin.close()


def test_hostenv_loop_is_the_same_with_sensitivity_on():
    """ddrl_eval_hostenv with sensitivity begun against a twin without: the same steps, episode
    table, filter statistics and last actions, bit for bit; the matrices cover the table's steps."""
    import torch
    n, E, limit, max_steps = 24, 2, 40, 100
    rng = np.random.default_rng(6)
    filt = S.filt(43, rng)
    eps = torch.from_numpy(rng.normal(size=(max_steps, n, 4, 2)).astype(np.float32)).cuda()
    out = []
    for sens in (False, True):
        ctx, cfg, inst = _ctx("QuantrupedMultiEnv_Local", n, None, frag=1)
        init_params(ctx, cfg, 9, head_scale=1.0)
        ctx.filter_set(*filt)
        env = N.HostEnv(n, 43, n_threads=2, seed=21)
        env.set_time_limit(limit)
        ctx.eval_begin(E, filter_update=True)
        if sens:
            ctx.eval_sens_begin([np.full(cfg.obs_dim[p], 0.1) for p in range(cfg.n_policies)])
        steps = ctx.eval_hostenv(env, eps, max_steps, max_steps, poll_every=5)
        res = [ctx.eval_sens_results(p) for p in range(cfg.n_policies)] if sens else None
        out.append((steps, ctx.eval_results(), ctx.filter_get(), env.act.copy(), res))
        ctx.eval_end()
        ctx.close()
        env.close()
    (sa, ta, fa, aa, _), (sb, tb, fb, ab, res) = out
    assert sa == sb and 1 < sa
    np.testing.assert_array_equal(ta, tb)
    np.testing.assert_array_equal(aa, ab)
    for x, y in zip(fa, fb):
        np.testing.assert_array_equal(x, y)
    assert not np.isnan(tb).any()
    for grads, grads_abs, rows in res:
        assert rows == int(tb[:, :, 1].sum())      # one base row per env step of the table's episodes (k = 1)
        assert (grads_abs > 0).mean() >= 0.9 and (np.abs(grads) <= grads_abs).all()


# ---- refusals -------------------------------------------------------------------------------
def test_refusals_give_messages():
    import ctypes
    import torch
    ctx, cfg, inst = _ctx("QuantrupedMultiEnv_Local", 4, None, frag=2)
    init_params(ctx, cfg, 1, head_scale=1.0)
    obs = torch.zeros((4, 43), dtype=torch.float32, device="cuda")
    act = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    hs = [np.full(cfg.obs_dim[p], 0.1) for p in range(cfg.n_policies)]
    with pytest.raises(N.DdrlError, match="ddrl_eval_begin first"):
        ctx.eval_sens_begin(hs)
    ctx.eval_begin(1)
    with pytest.raises(N.DdrlError, match="ddrl_eval_sens_begin first"):
        ctx.eval_sens(obs)
    with pytest.raises(N.DdrlError, match="ddrl_eval_sens_begin first"):
        ctx.eval_sens_results(0)
    with pytest.raises(N.DdrlError, match="null step"):
        N._ck(ctx.lib.ddrl_eval_sens_begin(ctx.h, None))
    tab = (ctypes.c_void_p * N.MAX_P)(*([hs[0].ctypes.data] + [None] * (N.MAX_P - 1)))
    with pytest.raises(N.DdrlError, match="null step"):
        N._ck(ctx.lib.ddrl_eval_sens_begin(ctx.h, tab))
    for bad in (-0.1, float("nan"), float("inf")):
        h = [a.copy() for a in hs]
        h[1][7] = bad
        with pytest.raises(N.DdrlError, match="finite"):
            ctx.eval_sens_begin(h)
    with pytest.raises(N.DdrlError, match="ddrl_eval_sens_begin first"):   # a refused begin leaves the mode off
        ctx.eval_sens(obs)
    ctx.eval_sens_begin(hs)
    with pytest.raises(N.DdrlError, match="ddrl_eval_act"):   # no eval_act since eval_begin
        ctx.eval_sens(obs)
    ctx.eval_act(obs, None, act)
    ctx.eval_sens(obs)
    ctx.filter_set(1.0, np.zeros(43), np.zeros(43))
    with pytest.raises(N.DdrlError, match="ddrl_eval_act"):   # the filter changed since
        ctx.eval_sens(obs)
    ctx.eval_act(obs, None, act)
    ctx.observe(obs)
    with pytest.raises(N.DdrlError, match="ddrl_eval_act"):   # an observe pushed into the filter
        ctx.eval_sens(obs)
    with pytest.raises(N.DdrlError, match="null"):
        ctx.eval_sens(None)
    with pytest.raises(N.DdrlError, match="bad policy"):
        ctx.eval_sens_results(7)
    ctx.eval_end()
    with pytest.raises(N.DdrlError, match="ddrl_eval_begin first"):
        ctx.eval_sens(obs)
    ctx.eval_begin(1)
    with pytest.raises(N.DdrlError, match="ddrl_eval_sens_begin first"):   # eval_end ended the mode
        ctx.eval_sens(obs)
    ctx.eval_end()
    ctx.close()


def test_graphnet_contexts_stay_refused():
    ctx, cfg, inst = _ctx(GNN_ENV, 8, None, frag=2)
    with pytest.raises(N.DdrlError, match="fcnet"):
        ctx.eval_begin(1)
    with pytest.raises(N.DdrlError, match="ddrl_eval_begin first"):
        ctx.eval_sens_begin([np.full(19, 0.1)])
    ctx.close()
