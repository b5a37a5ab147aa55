"""Uneven ground on the device env plane (the terrain instance of k_devenv_step, the probe kernel)
against the host env plane of the same library, and through the rollout, the evaluation loop and
the trainer.

The height field (csrc/envdyn.h, "terrain") is integer arithmetic, floor and + - * only, so the
device probe must equal the host probe -- itself bit-equal to tests/terrain_reference.py, see
tests/test_terrain_host.py -- bit for bit.  In the step, the field is evaluated at the foot's world
position, which contains sin(q_hip) * cos(q_knee): the last-place differences between glibc's and
the device library's sin / cos reach the ground height too, which is why the field has to be
continuous.  Resets, done flags and joints stay bit-equal as in tests/test_gpu_devenv.py; the torso
state and the foot forces get that file's bars, re-derived for uneven ground:

  * fp64 torso state and foot forces: 1e-10 * (1 + |host|).  tools/envdyn_nudge.cpp repeats that
    file's experiment on the CPU with terrain on and this test's inputs (seed 43, smoothness 0.6,
    states handed over at x = 10 m, 64 steps of full-amplitude scripted actions, time limit 50,
    D = 43 and 44): nudging every sin / cos result of the host dynamics by -1 / 0 / +1 ulp, 16 runs,
    moved them by at most 2.12e-13 at 65 envs and 1.45e-13 at 5 envs, with no done-flag and no
    contact-pattern mismatch (101 and 11 episode ends, 6316 and 472 foot contacts; the flat step
    under the same inputs: 1.03e-13).  Seed 43 is smooth as it stands: no touch-down flipped.  A
    library 4 ulp off scales the movement to about 8.5e-13, so the bar is 470 times the largest
    movement seen and more than 100 times the projected one;
  * the fp32 outputs the torso feeds: 2 fp32 ulp of the host's value, as in that file.

N in {5, 65}: 65 puts an env past the first 64-env workgroup; D in {43, 44}."""
import numpy as np
import pytest

from ddrl_amd import native as N
from tests import terrain_reference as R
from tests.gpu_harness import dev, init_params, make_ctx
from tests.test_gpu_devenv import (COL, LOCAL, TVS, _eval_ctx, _eval_stepwise, _stepwise_fragment, assert_bits,
                                   compare_step, script)

pytestmark = pytest.mark.gpu
SEED, LIMIT, SMOOTH = 43, 50, 0.6
SHAPES = [pytest.param(n, D, id=f"n{n}_d{D}") for n in (5, 65) for D in (43, 44)]
PTS = R.probe_points()


def make_pair(n, D):
    config = {"env_config": {"target_velocity": TVS}} if D == 44 else None
    ctx, cfg, inst = make_ctx(LOCAL, n, 1, config)
    tv = TVS if D == 44 else 0.0
    denv = N.DevEnv(ctx, seed=SEED, target_velocity=tv)
    henv = N.HostEnv(n, D, 2, SEED, tv)
    for env in (denv, henv):
        env.set_time_limit(LIMIT)
    return ctx, denv, henv


def at_x10(state):
    s = state.copy()
    s[:, 0] = 10.0
    s[:, 1] = -3.0 + 6.0 * np.arange(len(s)) / (len(s) - 1)
    return s


@pytest.mark.parametrize("n,D", SHAPES)
def test_device_probe_equals_the_host_probe(n, D):
    ctx, denv, henv = make_pair(n, D)
    denv.reset()
    henv.reset()
    for t in range(3):                       # a few envs are in their second episode: the field is keyed by it
        a = script(n, t)
        denv.step(dev(a))
        henv.act[:] = a
        henv.step()
    episodes = henv.state()[:, COL["episode"]]
    assert_bits(denv.state()[:, COL["episode"]], episodes, "episode numbers")
    assert denv.terrain == henv.terrain == {"lo": 1.0, "hi": 1.0, "bump_scale": 2.0, "generation": 0}
    idx = np.arange(len(PTS)) % n
    for lo, hi, bump, gen in ((0.0, 0.0, 2.0, 0), (0.6, 0.6, 2.0, 7), (1.0, 1.0, 2.0, 0), (0.6, 1.0, 1.7, 3)):
        for env in (denv, henv):
            env.set_terrain(lo, hi, bump, gen)
        assert denv.terrain == henv.terrain == {"lo": lo, "hi": hi, "bump_scale": bump, "generation": gen}
        for e in (0, n - 1, idx):
            hd, hh = denv.terrain_height(e, PTS), henv.terrain_height(e, PTS)
            assert_bits(hd, hh, f"probe lo={lo} hi={hi} gen={gen}")
        assert_bits(hh, R.heights(SEED, idx, lo, hi, bump, gen, episodes, PTS), "host probe against the reference")
        assert (hh > 0).any() == (lo < 1.0)
    for env in (denv, henv):
        env.new_terrain()
    assert denv.terrain["generation"] == henv.terrain["generation"] == 4
    assert_bits(denv.terrain_height(idx, PTS), henv.terrain_height(idx, PTS), "probe after new_terrain")
    for args, msg in (((0.8, 0.6), "lo <= hi"), ((0.5, 1.5), "hi <= 1"), ((0.5, 0.5, 0.0), "bump_scale")):
        with pytest.raises(N.DdrlError, match=msg):
            denv.set_terrain(*args)
    with pytest.raises(N.DdrlError, match="out of range"):
        denv.terrain_height(n, [[0.0, 0.0]])
    denv.close()
    with pytest.raises(N.DdrlError, match="closed"):
        denv.new_terrain()
    henv.close()
    ctx.close()


@pytest.mark.parametrize("n,D", SHAPES)
def test_free_running_parity_on_uneven_ground(n, D):
    ctx, denv, henv = make_pair(n, D)
    flat = N.HostEnv(n, D, 2, SEED, TVS if D == 44 else 0.0)
    flat.set_time_limit(LIMIT)
    for env in (henv, flat):
        env.reset()
    start = at_x10(henv.state())
    for env in (denv, henv, flat):
        env.set_state(start)
    for env in (denv, henv):
        env.set_terrain(SMOOTH)
    assert_bits(denv.state(), henv.state(), "handed-over state")
    ends, worst, differs = 0, 0.0, False
    for t in range(64):
        a = script(n, t)
        denv.step(dev(a))
        for env in (henv, flat):
            env.act[:] = a
            env.step()
        e, w = compare_step(ctx, denv, henv, f"step {t}")
        ends, worst = ends + e, max(worst, w)
        differs = differs or not np.array_equal(henv.state()[:, COL["foot"]], flat.state()[:, COL["foot"]])
    print(f"n={n} D={D}: {ends} episode ends, worst fp64 torso / foot difference {worst:.3e}")
    assert ends >= n                         # resets on the way (every env passes its TimeLimit once)
    assert differs                           # and the ground really was uneven
    denv.close()
    henv.close()
    flat.close()
    ctx.close()


# ---- rollout ---------------------------------------------------------------------------------
def _rollout_pair(n, T, D):
    config = {"env_config": {"target_velocity": TVS}} if D == 44 else None
    out = []
    for _ in range(2):
        ctx, cfg, inst = make_ctx(LOCAL, n, T, config)
        init_params(ctx, cfg, 5, head_scale=1.0)
        ctx.filter_set(1000.0, np.linspace(-0.5, 0.5, D), np.full(D, 2000.0))
        denv = N.DevEnv(ctx, seed=SEED, target_velocity=TVS if D == 44 else 0.0)
        denv.set_time_limit(LIMIT)
        out.append((ctx, cfg, denv))
    return out


def _fragments(n, T, D, smooth):
    """Three fragments (reset + hand-over to x = 10 m, a replay, one after new_terrain) by
    ddrl_rollout_devenv and by the stepwise calls; asserts they agree bit for bit and returns the
    records of every fragment."""
    import torch
    (a, cfg, env_a), (b, _, env_b) = _rollout_pair(n, T, D)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    eps = torch.randn((T, n, cfg.n_agents, cfg.act_dim), device="cuda", generator=gen)
    actions = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    for ctx, env in ((a, env_a), (b, env_b)):
        if smooth is not None:
            env.set_terrain(smooth)
        ctx.observe(env.reset())
        env.set_state(at_x10(env.state()))
    records = []
    for frag in range(3):
        if frag == 2:                        # between two fragments: a stale captured graph would show
            env_a.new_terrain()
            env_b.new_terrain()
        a.rollout_devenv(env_a, eps, reset=False)
        _stepwise_fragment(b, cfg, env_b, eps, actions, reset=False)
        for c in (a, b):
            c.gae()
            c.synchronize()
        recs = [a.records_get(p) for p in range(cfg.n_policies)]
        for p in range(cfg.n_policies):
            assert np.isfinite(recs[p]).all()
            assert_bits(recs[p], b.records_get(p), f"fragment {frag} records of policy {p}")
            assert_bits(a.last_values_get(p), b.last_values_get(p), f"fragment {frag} last_v of policy {p}")
        assert_bits(env_a.state(), env_b.state(), f"fragment {frag} env state")
        assert_bits(env_a.obs.cpu().numpy(), env_b.obs.cpu().numpy(), f"fragment {frag} last observation")
        records.append(recs)
    gens = env_a.terrain["generation"]
    for env in (env_a, env_b):
        env.close()
    a.close()
    b.close()
    return records, gens


@pytest.mark.parametrize("n,D", [pytest.param(5, 44, id="n5_d44"), pytest.param(65, 43, id="n65_d43")])
def test_fragment_with_terrain_equals_the_stepwise_calls(n, D, monkeypatch):
    T = 3
    got = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("DDRL_ROLLOUT_GRAPH", graph)      # read when a context is created
        got[graph], gens = _fragments(n, T, D, SMOOTH)
        assert gens == 1
    for frag in range(3):
        for ra, rb in zip(got["1"][frag], got["0"][frag]):
            assert_bits(ra, rb, f"fragment {frag}: graph replay against direct launches")
    monkeypatch.setenv("DDRL_ROLLOUT_GRAPH", "1")
    flat, _ = _fragments(n, T, D, None)
    for frag in range(3):
        assert any(not np.array_equal(ra, rf) for ra, rf in zip(got["1"][frag], flat[frag])), frag
    # new_terrain on flat ground changes nothing: the flat fragment 2 is what a fourth replay would be,
    # and on uneven ground the new generation shows in the records
    again, _ = _fragments(n, T, D, SMOOTH)
    for ra, rb in zip(got["1"][2], again[2]):
        assert_bits(ra, rb, "the same settings, the same bits")


def test_a_stale_graph_would_show(monkeypatch):
    """The fragment after new_terrain differs from the one a replay of the old capture would give:
    the same two fragments with and without the new_terrain between them."""
    import torch
    monkeypatch.setenv("DDRL_ROLLOUT_GRAPH", "1")
    n, T = 5, 3
    out = []
    for renew in (True, False):
        (a, cfg, env_a), (b, _, env_b) = _rollout_pair(n, T, 43)
        env_b.close()
        b.close()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(3)
        eps = torch.randn((T, n, cfg.n_agents, cfg.act_dim), device="cuda", generator=gen)
        env_a.set_terrain(SMOOTH)
        a.observe(env_a.reset())
        env_a.set_state(at_x10(env_a.state()))
        a.rollout_devenv(env_a, eps, reset=False)
        if renew:
            env_a.new_terrain()
        a.rollout_devenv(env_a, eps, reset=False)
        a.synchronize()
        out.append(env_a.state())
        env_a.close()
        a.close()
    assert not np.array_equal(out[0][:, COL["foot"]], out[1][:, COL["foot"]])


# ---- evaluation ------------------------------------------------------------------------------
def test_eval_loop_with_terrain_equals_the_stepwise_calls():
    n, E, poll, max_steps = 65, 2, 5, 40
    rng = np.random.default_rng(6)
    eps = dev(rng.normal(size=(max_steps, n, 4, 2)).astype(np.float32))
    tables = {}
    for smooth in (SMOOTH, 1.0):
        pair = []
        for _ in range(2):
            ctx, cfg = _eval_ctx(n)
            denv = N.DevEnv(ctx, seed=21)
            denv.set_time_limit(20)
            denv.set_terrain(smooth)
            ctx.eval_begin(E, filter_update=True)
            pair.append((ctx, denv))
        (ca, ea), (cb, eb) = pair
        steps_a = ca.eval_devenv(ea, eps, max_steps, max_steps, poll_every=poll)
        steps_b = _eval_stepwise(cb, eb, eps, max_steps, poll, False)
        assert steps_a == steps_b and 1 < steps_a <= max_steps
        tables[smooth] = ca.eval_results()
        assert_bits(tables[smooth], cb.eval_results(), "result table")
        assert_bits(ea.state(), eb.state(), "env state")
        for c, e in pair:
            c.eval_end()
            e.close()
            c.close()
    # 20 steps from the start patch: the feet reach the rim of the patch, where the ground rises
    assert not np.array_equal(tables[SMOOTH], tables[1.0])


def test_eval_table_with_terrain_against_the_host_plane():
    """test_eval_table_against_the_host_plane of tests/test_gpu_devenv.py with smoothness 0.6 on
    both planes: equal durations and written / NaN pattern, the other columns within its 1e-6
    relative (the table's inputs pass through fp32 before the fp64 sums)."""
    n, E, max_steps = 37, 2, 40
    rng = np.random.default_rng(8)
    eps = dev(rng.normal(size=(max_steps, n, 4, 2)).astype(np.float32))
    ca, _ = _eval_ctx(n)
    cb, _ = _eval_ctx(n)
    denv = N.DevEnv(ca, seed=21)
    henv = N.HostEnv(n, 43, n_threads=2, seed=21)
    for env in (denv, henv):
        env.set_time_limit(20)
        env.set_terrain(SMOOTH)
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
    rel = np.where(ta[:, :, cols] == tb[:, :, cols], 0.0, rel)
    print(f"device vs host evaluation table on uneven ground: largest relative difference {np.nanmax(rel):.3e}")
    np.testing.assert_allclose(ta[:, :, cols], tb[:, :, cols], rtol=1e-6, atol=0.0, equal_nan=True)
    for c in (ca, cb):
        c.eval_end()
    denv.close()
    henv.close()
    ca.close()
    cb.close()


# ---- trainer ---------------------------------------------------------------------------------
CURRICULUM = {"curriculum_learning": True, "range_smoothness": [1.0, 0.6], "range_last_timestep": 10_000}


@pytest.mark.parametrize("backend", ["host", "device"])
def test_trainer_sets_the_ground_and_the_hook_renews_it(backend):
    from ddrl_amd.trainer import PPOTrainer
    cfg = {"env": LOCAL, "env_backend": backend, "rollout_fragment_length": 16, "env_config": {"hf_smoothness": 0.8}}
    tr = PPOTrainer(cfg, n_envs=8, seed=3)
    assert tr.backend.terrain == {"lo": 0.8, "hi": 0.8, "bump_scale": 2.0, "generation": 0}
    r = tr.train()
    assert np.isfinite(r["episode_reward_mean"]) or r["episodes_this_iter"] == 0
    ts = r["timesteps_total"]
    tr.workers.foreach_worker(lambda w: w.foreach_env(lambda env: env.update_environment_after_epoch(ts)))
    assert tr.backend.terrain == {"lo": 0.8, "hi": 0.8, "bump_scale": 2.0, "generation": 1}
    assert (tr.backend.env.state()[:, COL["steps"]] == 0).all()
    tr.stop()
    # with the curriculum keys the callback moves the smoothness interval as the adaptor does
    tr = PPOTrainer({**cfg, "env_config": {"hf_smoothness": 1.0, **CURRICULUM}}, n_envs=8, seed=3)
    for k, (ts, lo) in enumerate([(0, 1.0), (5000, 0.8), (20_000, 0.6)]):
        tr.workers.foreach_worker(lambda w: w.foreach_env(lambda env: env.update_environment_after_epoch(ts)))
        t = tr.backend.terrain
        assert t["lo"] == pytest.approx(lo, abs=1e-15) and t["hi"] == 1.0 and t["generation"] == k + 1
    r = tr.train()                           # and training goes on over the interval's ground
    for st in r["info"]["learner"].values():
        assert all(np.isfinite(v) for v in st.values())
    tr.stop()


@pytest.mark.parametrize("backend", ["host", "device"])
def test_evaluate_on_uneven_ground(backend):
    from ddrl_amd.trainer import PPOTrainer
    cfg = {"env": LOCAL, "env_backend": backend, "rollout_fragment_length": 16, "env_config": {"hf_smoothness": 0.8}}
    tr = PPOTrainer(cfg, n_envs=8, seed=3)
    tr.train()
    before = (tr.backend.terrain, tr.backend.env.state().copy(), tr.ctx.params_get(0).copy(), tr.rctx.filter_get())
    args = dict(num_episodes=8, num_steps=40, explore=False, env_backend=backend, seed=5)
    frozen = dict(args)     # the default env_filter: a copy of the training filter, taken anew by every call
    rough = tr.evaluate(hf_smoothness=0.6, **frozen)
    assert tr.evaluate(hf_smoothness=0.6, **frozen) == rough            # reproducible for a seed
    flat = tr.evaluate(hf_smoothness=1.0, **frozen)
    assert flat != rough and len(rough[0]) == 8
    assert tr.evaluate(**frozen) == tr.evaluate(hf_smoothness=0.8, **frozen)   # the default: env_config's value
    lists, sens = tr.evaluate_sensitivity(num_episodes=8, num_steps=40, explore=False, env_backend=backend, seed=5,
                                          hf_smoothness=0.6)
    assert lists == rough and all(s["rows"] > 0 for s in sens.values())
    # the training context, its env plane and its terrain settings are untouched
    assert tr.backend.terrain == before[0]
    assert_bits(tr.backend.env.state(), before[1], "training env state")
    assert_bits(tr.ctx.params_get(0), before[2], "training weights")
    for x, y in zip(tr.rctx.filter_get(), before[3]):
        assert_bits(np.asarray(x, np.float64), np.asarray(y, np.float64), "training env-side filter")
    tr.stop()


def test_synthetic_backend_warns_once_that_it_has_no_ground(monkeypatch):
    import warnings

    from ddrl_amd import trainer as T
    monkeypatch.setattr(T, "_warned_synthetic_terrain", False)
    cfg = {"env": LOCAL, "rollout_fragment_length": 8, "env_config": {"hf_smoothness": 0.8}}
    with pytest.warns(UserWarning, match="synthetic env backend"):
        T.PPOTrainer(cfg, n_envs=8).stop()
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*synthetic env backend.*")   # the second trainer says nothing
        T.PPOTrainer(cfg, n_envs=8).stop()
        T.PPOTrainer({**cfg, "env_config": {}}, n_envs=8).stop()


def test_evaluate_checkpoints_rows_carry_the_ground_they_ran_on(tmp_path):
    from ddrl_amd.evaluation import evaluate_checkpoints
    from ddrl_amd.trainer import PPOTrainer
    cfg = {"env": LOCAL, "rollout_fragment_length": 16}
    tr = PPOTrainer(cfg, n_envs=8, seed=3)
    tr.train()
    path = tr.save_rllib(str(tmp_path))
    tr.stop()
    args = dict(num_episodes=6, num_steps=40, explore_during_rollout=False, env_filter="frozen", seed=5)
    rows = {s: evaluate_checkpoints(cfg, [path], "Local", hf_smoothness=s, **args) for s in (0.6, 1.0)}
    for s, rs in rows.items():
        assert len(rs) == 6 and all(r["evaluated_on"] == s and r["trained_on"] == "flat" for r in rs)
    assert [r["reward"] for r in rows[0.6]] != [r["reward"] for r in rows[1.0]]
    again = evaluate_checkpoints(cfg, [path], "Local", hf_smoothness=0.6, **args)
    assert again == rows[0.6]
