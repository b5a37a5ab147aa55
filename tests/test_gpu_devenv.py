"""The device env plane (ddrl_devenv_*, devenv.hip) against the host env plane of the same
library, stepped on the CPU with the same seed and the same scripted actions.

Both planes run one source (csrc/envdyn.h).  Integer arithmetic, the reset hash and + - * / are
IEEE on both sides and the device kernels are built without fp contraction, so everything that
no sin / cos result reaches must be bit-equal: the resets, the done flags, the joint state and
the outputs it feeds.  The torso and the foot forces take sin / cos of the platform's libraries
(glibc here, the device library there) and get bars instead:

  * fp64 torso state and foot forces: 1e-10 * (1 + |host|).  Nudging every sin / cos result of the
    host dynamics by -1 / 0 / +1 ulp moved them by at most 1.4e-13 over 200 steps of this kind of
    input (64 envs, amplitude 1 and 0.3, time limits 1000 and 20; no done or contact-pattern
    mismatch); a library 4 ulp off scales that to about 6e-13, so the bar is more than 100 times
    the projected spread;
  * the fp32 outputs the torso feeds: 2 fp32 ulp of the host's value, 1 ulp being the spacing at
    max(|host|, 1e-6) (one rounding boundary crossed, plus one for a sin in a foot row).

Script: seed 43, actions a[e][t][j] uniform in [-1, 1) from a counter hash (full amplitude),
time_limit 20 -- episodes end constantly, by the TimeLimit and by the torso height.
N in {37: ragged quad lanes across a wave boundary, 64: one block, 65: the first env of a second
block}; D in {43, 44 with the target-velocity list [0.5, 1.0, 2.0]}."""
import ctypes as C

import numpy as np
import pytest

from ddrl_amd import native as N
from tests import episodes_reference as R
from tests.gpu_harness import dev, init_gnn_params, init_params, make_ctx

pytestmark = pytest.mark.gpu
LOCAL = "QuantrupedMultiEnv_Local"
SEED, LIMIT = 43, 20
TVS = [0.5, 1.0, 2.0]
SHAPES = [pytest.param(n, D, id=f"n{n}_d{D}") for n in (37, 64, 65) for D in (43, 44)]
COL = N.ENV_STATE_COLUMNS
JOINT_OBS = np.r_[5:13, 19:27, 27:35, 35:43]       # joint angles, joint velocities, forces, ctrl
TORSO_OBS = np.r_[0:5, 13:19]


def script(n, t, seed=SEED):
    """a[e][t][j] in [-1, 1): a splitmix-style hash of the counters (no state, any order)."""
    e, j = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(8, dtype=np.uint64), indexing="ij")
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) ^ (e * np.uint64(0x9E3779B97F4A7C15)) ^ (np.uint64(t) * np.uint64(0xBF58476D1CE4E5B9)) ^
             (j * np.uint64(0x94D049BB133111EB))) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return ((z >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0).astype(np.float32)


def make_pair(n, D, T=1):
    config = {"env_config": {"target_velocity": TVS}} if D == 44 else None
    ctx, cfg, inst = make_ctx(LOCAL, n, T, config)
    assert cfg.obs_full_dim == D
    tv = TVS if D == 44 else 0.0
    denv = N.DevEnv(ctx, seed=SEED, target_velocity=tv)
    henv = N.HostEnv(n, D, 2, SEED, tv)
    denv.set_time_limit(LIMIT)
    henv.set_time_limit(LIMIT)
    return ctx, denv, henv


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def assert_bits(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def assert_ulp32(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(1e-6)).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.isfinite(got).all() and (err <= 2.0 * ulp).all(), f"{what}: {float((err / ulp).max())} ulp"


def assert_f64(got, want, what):
    err = np.abs(got - want) / (1.0 + np.abs(want))
    assert np.isfinite(got).all() and (err <= 1e-10).all(), f"{what}: {float(err.max())}"
    return float(err.max())


def device_outputs(ctx, denv):
    ctx.synchronize()
    return {k: getattr(denv, k).cpu().numpy() for k in ("obs", "fw", "cfrc", "kin", "done")}


def compare_step(ctx, denv, henv, what):
    """Every env, every output and the whole state of one step, by the module docstring's rules."""
    d = device_outputs(ctx, denv)
    np.testing.assert_array_equal(d["done"], henv.done, err_msg=f"{what} done")
    assert_bits(d["obs"][:, JOINT_OBS], henv.obs[:, JOINT_OBS], f"{what} joint obs columns")
    if henv.obs_dim == 44:
        assert_bits(d["obs"][:, 43], henv.obs[:, 43], f"{what} target velocity column")
    assert_bits(d["kin"][:, 1:], henv.kin[:, 1:], f"{what} kin joint velocities")
    assert_ulp32(d["obs"][:, TORSO_OBS], henv.obs[:, TORSO_OBS], f"{what} torso obs columns")
    assert_ulp32(d["fw"], henv.fw, f"{what} fw")
    assert_ulp32(d["cfrc"], henv.cfrc, f"{what} cfrc")
    assert_ulp32(d["kin"][:, 0], henv.kin[:, 0], f"{what} kin dx")
    sd, sh = denv.state(), henv.state()
    for k in ("q", "qd", "qfrc", "steps", "episode", "tv"):
        assert_bits(sd[:, COL[k]], sh[:, COL[k]], f"{what} state {k}")
    worst = max(assert_f64(sd[:, COL["torso"]], sh[:, COL["torso"]], f"{what} torso state"),
                assert_f64(sd[:, COL["foot"]], sh[:, COL["foot"]], f"{what} foot forces"))
    return int(henv.done.sum()), worst


def step_both(ctx, denv, henv, t):
    a = script(henv.n, t)
    denv.step(dev(a))
    henv.act[:] = a
    henv.step()


@pytest.mark.parametrize("n,D", SHAPES)
def test_resets_are_bit_equal(n, D):
    ctx, denv, henv = make_pair(n, D)

    def same(what):
        d = device_outputs(ctx, denv)
        assert_bits(denv.state(), henv.state(), f"{what} state")
        assert_bits(d["obs"], henv.obs, f"{what} obs")
        assert_bits(d["done"], henv.done, f"{what} done")
        assert_bits(denv.target_velocities, henv.target_velocities, f"{what} target velocities")

    denv.reset()
    henv.reset()
    same("reset")
    s = henv.state()
    assert len(np.unique(s[:, COL["steps"]])) > 1 and (s[:, COL["episode"]] == 1).all()   # staggered phases
    if D == 44:
        assert set(np.unique(henv.target_velocities)) == set(np.float32(TVS))
    for t in range(6):                       # into the episodes, a few of them over
        step_both(ctx, denv, henv, t)
    before = device_outputs(ctx, denv)
    tv_before = denv.target_velocities
    denv.reset_state()
    henv.reset_state()
    after = device_outputs(ctx, denv)
    assert_bits(denv.state(), henv.state(), "reset_state state")
    assert (denv.state()[:, COL["steps"]] == 0).all()
    for k in ("obs", "done"):                # reset_state leaves obs / done / tv untouched
        assert_bits(after[k], before[k], f"reset_state {k}")
    assert_bits(denv.target_velocities, tv_before, "reset_state target velocities")
    denv.reset_episodes()
    henv.reset_episodes()
    same("reset_episodes")
    assert (denv.state()[:, COL["steps"]] == 0).all()
    denv.close()
    henv.close()
    ctx.close()


@pytest.mark.parametrize("n,D", SHAPES)
def test_free_running_parity(n, D):
    ctx, denv, henv = make_pair(n, D)
    denv.reset()
    henv.reset()
    ends, worst = 0, 0.0
    for t in range(64):
        step_both(ctx, denv, henv, t)
        e, w = compare_step(ctx, denv, henv, f"step {t}")
        ends, worst = ends + e, max(worst, w)
    print(f"n={n} D={D}: {ends} episode ends, worst fp64 torso / foot difference {worst:.3e}")
    assert ends >= 2 * n                     # resets were exercised all along
    denv.close()
    henv.close()
    ctx.close()


@pytest.mark.parametrize("n,D", [pytest.param(37, 43, id="n37_d43"), pytest.param(65, 44, id="n65_d44")])
def test_hand_over_from_a_running_host_env(n, D):
    ctx, denv, henv = make_pair(n, D)
    henv.reset()
    for t in range(30):
        henv.act[:] = script(n, t)
        henv.step()
    denv.set_state(henv.state())
    assert_bits(denv.state(), henv.state(), "handed-over state")
    for t in range(30, 40):
        step_both(ctx, denv, henv, t)
        compare_step(ctx, denv, henv, f"step {t} after the hand-over")
    denv.close()
    henv.close()
    ctx.close()


# ---- rollout ---------------------------------------------------------------------------------
ROLLOUT_CASES = [
    pytest.param(LOCAL, None, id="local"),
    pytest.param("QuantrupedMultiEnv_SharedDecentral", {"observation_filter": "MeanStdFilter"}, id="shared_pfilter"),
    pytest.param("QuantrupedMultiEnv_FullyDecentral", {"env_config": {"target_velocity": TVS}}, id="tvel"),
    pytest.param("QuantrupedMultiEnv_DecentralShared_Graph", None, id="graphnet"),
]


def _rollout_ctx(env_name, config, n, T):
    ctx, cfg, inst = make_ctx(env_name, n, T, config)
    gnn = cfg.model_kind == N.MODEL_GNN
    if gnn:
        init_gnn_params(ctx, 5, head_scale=1.0)
    else:
        init_params(ctx, cfg, 5, head_scale=1.0)
    ctx.filter_set(1000.0, np.linspace(-0.5, 0.5, cfg.obs_full_dim), np.full(cfg.obs_full_dim, 2000.0))
    tv = ((config or {}).get("env_config") or {}).get("target_velocity", 0.0)
    denv = N.DevEnv(ctx, seed=SEED, target_velocity=tv)
    denv.set_time_limit(LIMIT)
    return ctx, cfg, denv, gnn


def _stepwise_fragment(ctx, cfg, denv, eps, actions, reset):
    """The public calls ddrl_rollout_devenv stands for, one by one; returns the done flags [T][N]."""
    if reset:
        ctx.observe(denv.reset())
    done = []
    for t in range(cfg.frag_len):
        ctx.act(t, eps[t], actions)
        denv.step(actions)
        ctx.reward(t, denv.fw, denv.cfrc, actions, denv.done)
        ctx.observe(denv.obs)
        ctx.synchronize()
        done.append(denv.done.cpu().numpy().copy())
    ctx.bootstrap()
    return np.stack(done)


@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "launches"])
@pytest.mark.parametrize("env_name,config", ROLLOUT_CASES)
def test_rollout_equals_the_stepwise_calls(env_name, config, graph, monkeypatch):
    import torch
    monkeypatch.setenv("DDRL_ROLLOUT_GRAPH", graph)      # read when a context is created
    n, T = 37, 5
    a, cfg, env_a, _ = _rollout_ctx(env_name, config, n, T)
    b, _, env_b, _ = _rollout_ctx(env_name, config, n, T)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    eps = torch.randn((T, n, cfg.n_agents, cfg.act_dim), device="cuda", generator=gen)
    actions = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    ref = R.EpisodeReference(n, cfg.n_agents)
    ends = 0
    # fragment 0 resets, 1 continues (a replay of the captured loop), 2 runs under another TimeLimit
    # (a setting the captured launches hold: the loop has to be captured again)
    for frag in range(3):
        if frag == 2:
            env_a.set_time_limit(3)
            env_b.set_time_limit(3)
        a.rollout_devenv(env_a, eps, reset=frag == 0)
        done = _stepwise_fragment(b, cfg, env_b, eps, actions, reset=frag == 0)
        rows_a, rows_b = a.episodes_collect(), b.episodes_collect()
        np.testing.assert_array_equal(rows_a, rows_b)
        # done_tn: the rows sit at exactly the (t, env) of the env plane's done flags
        np.testing.assert_array_equal(rows_a[:, :2], np.argwhere(done).astype(np.float64))
        # returns are the fp64 sums of the records' fp32 rewards (test_gpu_episodes.py), every model kind
        np.testing.assert_array_equal(rows_a, ref.fragment(R.record_rewards(a, cfg), done))
        np.testing.assert_array_equal(a.episodes_inflight(), ref.inflight())
        ends += len(rows_a)
        for c in (a, b):
            c.gae()                           # advantages and value targets read done_tn
            c.synchronize()
        for p in range(cfg.n_policies):
            ra = a.records_get(p)
            assert np.isfinite(ra).all()
            assert_bits(ra, b.records_get(p), f"fragment {frag} records of policy {p}")
            assert_bits(a.last_values_get(p), b.last_values_get(p), f"fragment {frag} last_v of policy {p}")
            if cfg.policy_filter:
                for x, y in zip(a.policy_filter_get(p), b.policy_filter_get(p)):
                    assert_bits(np.asarray(x, np.float64), np.asarray(y, np.float64), "per-policy filter")
        for x, y in zip(a.filter_get(), b.filter_get()):
            assert_bits(np.asarray(x, np.float64), np.asarray(y, np.float64), f"fragment {frag} env-side filter")
        assert_bits(env_a.state(), env_b.state(), f"fragment {frag} env state")
        assert_bits(env_a.obs.cpu().numpy(), env_b.obs.cpu().numpy(), f"fragment {frag} last observation")
    assert a.filter_get()[0] == 1000.0 + n * (3 * T + 1)
    assert ends >= n // 2                     # episodes ended inside the fragments
    for env in (env_a, env_b):
        env.close()
    a.close()
    b.close()


# ---- evaluation ------------------------------------------------------------------------------
def _eval_ctx(n, seed=9):
    ctx, cfg, inst = make_ctx(LOCAL, n, 1)
    init_params(ctx, cfg, seed, head_scale=1.0)
    rng = np.random.default_rng(6)
    ctx.filter_set(100.0, rng.normal(size=43) * 0.1, np.abs(rng.normal(size=43)) * 99 + 1)
    return ctx, cfg


def _eval_stepwise(ctx, denv, eps, max_steps, poll, sens):
    import torch
    n = denv.n
    actions = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    denv.reset_episodes()
    steps = 0
    while steps < max_steps:
        ctx.eval_act(denv.obs, eps[steps] if eps is not None else None, actions)
        if sens:
            ctx.eval_sens(denv.obs)
        denv.step(actions)
        ctx.eval_step(denv.fw, denv.cfrc, actions, denv.kin, denv.done)
        ctx.synchronize()
        steps += 1
        if steps % poll == 0 and ctx.eval_progress()[1] == n:
            break
    return steps


@pytest.mark.parametrize("explore,sens", [(False, False), (True, False), (True, True)],
                         ids=["deterministic", "noise", "noise_sensitivity"])
def test_eval_loop_equals_the_stepwise_calls(explore, sens):
    import torch
    n, E, poll, max_steps = 37, 2, 5, 2 * LIMIT
    rng = np.random.default_rng(6)
    eps = dev(rng.normal(size=(max_steps, n, 4, 2)).astype(np.float32)) if explore else None
    pair = []
    for _ in range(2):
        ctx, cfg = _eval_ctx(n)
        denv = N.DevEnv(ctx, seed=21)
        denv.set_time_limit(LIMIT)
        ctx.eval_begin(E, filter_update=True)
        if sens:
            ctx.eval_sens_begin([np.full(cfg.obs_dim[p], 0.1) for p in range(cfg.n_policies)])
        pair.append((ctx, denv))
    (ca, ea), (cb, eb) = pair
    steps_a = ca.eval_devenv(ea, eps, max_steps if explore else 0, max_steps, poll_every=poll)
    steps_b = _eval_stepwise(cb, eb, eps, max_steps, poll, sens)
    assert steps_a == steps_b and 1 < steps_a <= E * LIMIT
    ta, tb = ca.eval_results(), cb.eval_results()
    assert_bits(ta, tb, "result table")
    assert not np.isnan(ta[:, :, :5]).any() and ca.eval_progress() == cb.eval_progress() == (n * E, n)
    assert ta[:, :, 1].max() <= LIMIT and ta[:, :, 1].min() >= 1
    for x, y in zip(ca.filter_get(), cb.filter_get()):
        assert_bits(np.asarray(x, np.float64), np.asarray(y, np.float64), "env-side filter")
    if sens:
        for p in range(cfg.n_policies):
            ga, gaa, ra = ca.eval_sens_results(p)
            gb, gab, rb = cb.eval_sens_results(p)
            assert ra == rb > 0 and np.abs(ga).sum() > 0
            assert_bits(ga, gb, f"grads of policy {p}")
            assert_bits(gaa, gab, f"grads_abs of policy {p}")
    assert_bits(ea.state(), eb.state(), "env state")
    for c, e in pair:
        c.eval_end()
        e.close()
        c.close()


def test_eval_table_against_the_host_plane():
    """The device loop and ddrl_eval_hostenv over a host plane of the same seed: frozen filter,
    num_steps 20.  Durations and the written / NaN row pattern are equal; the other columns are
    within 1e-6 relative -- a loose outer bar: the table's inputs pass through fp32 (fw, cfrc, kin)
    before the fp64 sums, and one 1-ulp fp32 difference in one of 20 terms is about 6e-8 of that
    term.  The observed maximum is printed."""
    n, E, max_steps = 37, 2, 2 * LIMIT
    rng = np.random.default_rng(8)
    eps = dev(rng.normal(size=(max_steps, n, 4, 2)).astype(np.float32))
    ca, _ = _eval_ctx(n)
    cb, _ = _eval_ctx(n)
    denv = N.DevEnv(ca, seed=21)
    henv = N.HostEnv(n, 43, n_threads=2, seed=21)
    for env in (denv, henv):
        env.set_time_limit(LIMIT)
    for c in (ca, cb):
        c.eval_begin(E, filter_update=False)
    sa = ca.eval_devenv(denv, eps, max_steps, max_steps, poll_every=5)
    sb = cb.eval_hostenv(henv, eps, max_steps, max_steps, poll_every=5)
    ta, tb = ca.eval_results(), cb.eval_results()
    assert sa == sb
    np.testing.assert_array_equal(ta[:, :, 1], tb[:, :, 1])                 # duration
    np.testing.assert_array_equal(np.isnan(ta), np.isnan(tb))               # written / NaN pattern
    assert not np.isnan(tb[:, :, 1]).any()
    cols = [0, 2, 3, 4, 5]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(ta[:, :, cols] - tb[:, :, cols]) / np.abs(tb[:, :, cols])
    rel = np.where(ta[:, :, cols] == tb[:, :, cols], 0.0, rel)              # equal values (0, inf) differ by nothing
    print(f"device vs host evaluation table: largest relative difference {np.nanmax(rel):.3e}")
    np.testing.assert_allclose(ta[:, :, cols], tb[:, :, cols], rtol=1e-6, atol=0.0, equal_nan=True)
    for c in (ca, cb):
        c.eval_end()
    denv.close()
    henv.close()
    ca.close()
    cb.close()


def test_eval_table_grows_between_sessions():
    """ddrl_eval_begin keeps the result table between sessions and replaces it when a session asks for more
    episodes per env: 1, then 3, on one context (a new env plane of the same seed per session, so both sessions
    start from the same env state).  The second session's table is, bit for bit, the one a fresh context writes
    that is run with 3 directly."""
    n, limit = 16, 4
    tables = []
    for sessions in ((1, 3), (3,)):
        ctx, _ = _eval_ctx(n)
        for E in sessions:
            denv = N.DevEnv(ctx, seed=21)
            denv.set_time_limit(limit)
            ctx.eval_begin(E, filter_update=False)
            steps = ctx.eval_devenv(denv, max_steps=2 * E * limit, poll_every=2)
            table = ctx.eval_results()
            assert table.shape == (n, E, 6) and 1 < steps <= E * limit and ctx.eval_progress() == (n * E, n)
            assert not np.isnan(table[:, :, :5]).any()
            ctx.eval_end()
            denv.close()
        tables.append(table)
        ctx.close()
    assert_bits(tables[0], tables[1], "result table of the grown session")


# ---- messages --------------------------------------------------------------------------------
def test_refusals_have_messages():
    import torch
    n = 4
    ctx, cfg, _ = make_ctx(LOCAL, n, 2)
    other, _, _ = make_ctx(LOCAL, n, 2)
    tctx, _, _ = make_ctx(LOCAL, n, 2, {"env_config": {"target_velocity": [1.0]}})
    lib = ctx.lib
    denv, theirs = N.DevEnv(ctx, seed=1), N.DevEnv(other, seed=1)
    buf = torch.zeros((2, n, 4, 2), dtype=torch.float32, device="cuda")
    h = N.VP()
    f1 = (C.c_float * 1)(1.0)
    st = np.zeros(n * N.ENV_STATE_DOUBLES)
    null_calls = [lambda: lib.ddrl_devenv_step(None, buf.data_ptr()), lambda: lib.ddrl_devenv_reset(None),
                  lambda: lib.ddrl_devenv_reset_episodes(None), lambda: lib.ddrl_devenv_reset_state(None),
                  lambda: lib.ddrl_devenv_set_time_limit(None, 5),
                  lambda: lib.ddrl_devenv_set_target_velocities(None, f1, 1),
                  lambda: lib.ddrl_devenv_target_velocities(None, f1, 1),
                  lambda: lib.ddrl_devenv_buffers(None, None, None, None, None, None),
                  lambda: lib.ddrl_devenv_state_get(None, st.ctypes.data, st.size),
                  lambda: lib.ddrl_devenv_state_set(None, st.ctypes.data, st.size),
                  lambda: lib.ddrl_rollout_devenv(ctx.h, None, buf.data_ptr(), 0)]
    for call in null_calls:
        with pytest.raises(N.DdrlError, match="null device env"):
            N._ck(call())
    with pytest.raises(N.DdrlError, match="null context"):
        N._ck(lib.ddrl_devenv_create(None, 0, 0.0, C.byref(h)))
    with pytest.raises(N.DdrlError, match="null context"):
        N._ck(lib.ddrl_rollout_devenv(None, denv.h, buf.data_ptr(), 0))
    with pytest.raises(N.DdrlError, match="target_velocity > 0"):
        N.DevEnv(tctx, seed=1, target_velocity=0.0)
    with pytest.raises(N.DdrlError, match="another context"):
        ctx.rollout_devenv(theirs, buf)
    with pytest.raises(N.DdrlError, match="ddrl_eval_begin first"):
        ctx.eval_devenv(denv)
    ctx.eval_begin(1)
    with pytest.raises(N.DdrlError, match="another context"):
        ctx.eval_devenv(theirs)
    with pytest.raises(N.DdrlError, match="null device env"):
        N._ck(lib.ddrl_eval_devenv(ctx.h, None, None, 0, 10, 5, None))
    with pytest.raises(N.DdrlError, match="max_steps"):
        ctx.eval_devenv(denv, max_steps=0)
    with pytest.raises(N.DdrlError, match="eps_steps"):
        ctx.eval_devenv(denv, buf, eps_steps=0)
    ctx.eval_end()
    with pytest.raises(N.DdrlError, match="null noise buffer"):
        ctx.rollout_devenv(denv, None)
    with pytest.raises(N.DdrlError, match="null actions"):
        denv.step(None)
    with pytest.raises(N.DdrlError, match="n >= 1"):
        denv.set_target_velocities([])
    for bad in (float("nan"), float("inf")):
        with pytest.raises(N.DdrlError, match="finite"):
            denv.set_target_velocities([1.0, bad])
    tenv = N.DevEnv(tctx, seed=1, target_velocity=1.0)
    with pytest.raises(N.DdrlError, match="target velocities > 0"):
        tenv.set_target_velocities([1.0, 0.0])
    with pytest.raises(N.DdrlError, match="target velocities > 0"):
        N.DevEnv(tctx, seed=1, target_velocity=[1.0, -2.0])
    with pytest.raises(N.DdrlError, match="steps >= 1"):
        denv.set_time_limit(0)
    with pytest.raises(N.DdrlError, match="n_envs floats"):
        N._ck(lib.ddrl_devenv_target_velocities(denv.h, f1, 1))
    with pytest.raises(N.DdrlError, match="DDRL_ENV_STATE_DOUBLES"):
        denv.set_state(st[:-1])
    st[N.ENV_STATE_COLUMNS["episode"]] = 0.5
    with pytest.raises(N.DdrlError, match="non-negative integers"):
        denv.set_state(st)
    # use after close; an env whose context went first
    denv.close()
    for call in (denv.reset, denv.reset_episodes, denv.reset_state, lambda: denv.step(buf), denv.state,
                 lambda: denv.set_time_limit(5), lambda: denv.target_velocities):
        with pytest.raises(N.DdrlError, match="closed"):
            call()
    other.close()
    with pytest.raises(N.DdrlError, match="context has been destroyed"):
        theirs.reset()
    theirs.close()
    tenv.close()
    tctx.close()
    ctx.close()
