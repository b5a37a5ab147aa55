"""The group rollout (ddrl_rollout_group_*, csrc/rollout_group.hip): the device-plane fragments of M
contexts as one chain of launches with the member in the grid (needs an MI355X).

Contract: bitwise.  Member m of a group run leaves what ddrl_rollout_devenv leaves on a twin -- a
context and device env built by the same recipe, so holding the same parameters, env-side filter,
per-policy filters, env seed, packed env state, target velocities, terrain and time limit -- that
runs the plain chain on the same noise.  The members differ from each other in all of that.
The shapes are the smallest at which each kernel leaves its first unit: a partial act tile, a
second act workgroup and env-step block (64 envs per block), a workgroup boundary inside an env's
rows, a second, ragged filter chunk (256 rows per chunk)."""
import numpy as np
import pytest

from ddrl_amd import native as N
from tests.gpu_harness import CUP_CONFIG, CUP_ENV, GNN_ENV, init_cup_params, init_gnn_params, init_params, make_ctx

pytestmark = pytest.mark.gpu
LOCAL = "QuantrupedMultiEnv_Local"
SHARED = "QuantrupedMultiEnv_SharedDecentral"
CENTRAL = "QuantrupedMultiEnv_Centralized"
TWOSIDES = "QuantrupedMultiEnv_TwoSides"
PFILTER = {"observation_filter": "MeanStdFilter"}
TVS = [0.5, 1.0, 2.0]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def noise(shape, seed):
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=gen)


class Member:
    """A context and its device env made by a recipe keyed by the member index m: calling it twice
    gives two objects in the same state (the plain kernels are deterministic), a member and its
    twin.  The recipe ends with a plain warm-up fragment from a reset, so the state the compared
    fragment starts from is mid-episode: filters pushed, stages filled, envs apart."""

    def __init__(self, env_name, config, n, T, m, limit=1000, tvs=None, smooth=None, warm=True, gnn=False,
                 tv_env=False):
        self.ctx, self.cfg, _ = make_ctx(env_name, n, T, config)
        ctx, cfg = self.ctx, self.cfg
        if gnn:
            init_gnn_params(ctx, 5 + m, head_scale=1.0)
        elif cfg.leg_coupling:
            init_cup_params(ctx, cfg, 5 + m, head_scale=1.0)
        else:
            init_params(ctx, cfg, 5 + m, head_scale=1.0)
        rng = np.random.default_rng(100 + m)
        D = cfg.obs_full_dim
        ctx.filter_set(1000.0 + 10 * m, rng.normal(size=D) * 0.3, np.abs(rng.normal(size=D)) * 999.0 + 500.0)
        if cfg.policy_filter:
            for p in range(cfg.n_policies):
                d = cfg.obs_dim[p]
                ctx.policy_filter_set(p, 50.0 + m, rng.normal(size=d) * 0.1, np.abs(rng.normal(size=d)) * 40.0 + 20.0)
        self.env = N.DevEnv(ctx, seed=77 + 13 * m, target_velocity=[v + 0.25 * m for v in tvs] if tvs else 0.0)
        self.env.set_time_limit(limit + m)
        self.tv_table = None
        if tv_env:   # a fixed velocity per env, the member's own table; no entry is in the member's list
            self.tv_table = (1.0 + 0.25 * m + 0.01 * (np.arange(n) + 1)).astype(np.float32)
            self.env.set_env_target_velocities(self.tv_table)
        if smooth is not None:   # member 0 at `smooth`, the others over a range below it, each its own generation
            self.env.set_terrain(smooth - 0.05 * m, smooth, generation=3 + m)
        else:
            self.env.set_terrain(1.0, generation=m)   # flat whatever the generation
        if warm:
            ctx.rollout_devenv(self.env, noise((T, n, cfg.n_agents, cfg.act_dim), 900 + m), reset=True)
            ctx.gae()
            ctx.episodes_collect()
        ctx.synchronize()

    def snapshot(self, fragment=True):
        """Everything the fragment writes (fragment=True) or must leave alone."""
        ctx, cfg, out = self.ctx, self.cfg, {}
        ctx.synchronize()
        if not fragment:
            for p in range(cfg.n_policies):
                out[f"params{p}"] = ctx.params_get(p)
                m_, v_, b1, b2 = ctx.adam_get(p)
                out[f"adam{p}"] = np.concatenate([m_, v_, np.array([b1, b2], np.float32)])
                out[f"adv_norm{p}"] = np.asarray(ctx.adv_norm_get(p), np.float32)
            out["terrain"] = np.array([float(v) for v in self.env.terrain.values()])
            return out
        for p in range(cfg.n_policies):
            out[f"records{p}"] = ctx.records_get(p)
            out[f"last_v{p}"] = ctx.last_values_get(p)
            if cfg.policy_filter:
                for delta in (False, True):
                    n, M, S = ctx.policy_filter_get(p, delta=delta)
                    out[f"pfilter{p}_{int(delta)}"] = np.concatenate([[n], M, S]).astype(np.float64)
        for name, (n, M, S) in (("filter", ctx.filter_get()), ("filter_delta", ctx.filter_delta_get())):
            out[name] = np.concatenate([[n], M, S]).astype(np.float64)
        out["env_state"] = self.env.state()
        out["env_obs"] = self.env.obs.cpu().numpy()
        out["env_done"] = self.env.done.cpu().numpy()
        return out

    def after_gae(self):
        ctx, cfg, out = self.ctx, self.cfg, {}
        ctx.gae()
        out["episodes"] = np.asarray(ctx.episodes_collect(), np.float64)
        out["inflight"] = np.asarray(ctx.episodes_inflight(), np.float64)
        for p in range(cfg.n_policies):
            out[f"records{p}"] = ctx.records_get(p)
            out[f"adv_sums{p}"] = np.asarray(ctx.adv_sums_get(p), np.float64)
        return out

    def close(self):
        self.env.close()
        self.ctx.close()


def assert_same(got, want, what):
    assert list(got) == list(want), what
    for k in got:
        assert_bits(got[k], want[k], f"{what}: {k}")


def assert_members_differ(members, env_too=True):
    """Every pair of members differs in parameters, filters, env state and env settings.  env_too
    False: envs that were never reset hold no state yet (the run's reset draws it from their seeds)."""
    snaps = [(m.snapshot(True), m.snapshot(False)) for m in members]
    for i in range(len(members)):
        for j in range(i):
            (fi, oi), (fj, oj) = snaps[i], snaps[j]
            keys = ["filter"] + (["env_state", "env_obs"] if env_too else [])
            for k in keys + [k for k in fi if k.startswith("pfilter") and k.endswith("_0")]:
                assert not np.array_equal(fi[k], fj[k]), (i, j, k)
            assert not np.array_equal(oi["params0"], oj["params0"]), (i, j)
            assert members[i].env.terrain != members[j].env.terrain, (i, j)


def run_case(env_name, config, M, n, T, runs=1, reset=False, between=None, **kw):
    """Group run(s) against the twins' plain runs; returns the members' done flags per run."""
    members = [Member(env_name, config, n, T, m, **kw) for m in range(M)]
    twins = [Member(env_name, config, n, T, m, **kw) for m in range(M)]
    cfg = members[0].cfg
    for a, b in zip(members, twins):
        assert_same(a.snapshot(), b.snapshot(), "a twin starts in its member's state")
    if M > 1:
        assert_members_differ(members, env_too=kw.get("warm", True))
    outside = [a.snapshot(False) for a in members]
    group = N.RolloutGroup([a.ctx for a in members], [a.env for a in members])
    dones = []
    for run in range(runs):
        if between is not None and run:
            for m, (a, b) in enumerate(zip(members, twins)):
                between(a.env, m)
                between(b.env, m)
            outside = [a.snapshot(False) for a in members]
        eps = [noise((T, n, cfg.n_agents, cfg.act_dim), 10 * run + m) for m in range(M)]
        group.run(eps, reset=reset and run == 0)
        for b, e in zip(twins, eps):
            b.ctx.rollout_devenv(b.env, e, reset=reset and run == 0)
        for m, (a, b) in enumerate(zip(members, twins)):
            got = a.snapshot()
            assert all(np.isfinite(got[f"records{p}"]).all() for p in range(cfg.n_policies))
            assert_same(got, b.snapshot(), f"run {run} member {m}")
            assert_same(a.snapshot(False), outside[m], f"run {run} member {m}: state outside the fragment")
            ga, gb = a.after_gae(), b.after_gae()
            assert_same(ga, gb, f"run {run} member {m} after gae and episodes_collect")
            dones.append((run, m, ga["episodes"]))
            if a.tv_table is not None:   # the restarts read the table and drew nothing from the list
                np.testing.assert_array_equal(a.env.target_velocities, a.tv_table, err_msg=f"run {run} member {m}")
        if M > 1:
            assert_members_differ(members)
    group.close()
    for x in members + twins:
        x.close()
    return dones


@pytest.mark.parametrize("n", [8, 70])
@pytest.mark.parametrize("config", [None, PFILTER], ids=["nofilter", "pfilter"])
def test_local_three_members(n, config):
    """n = 8: one partial act tile.  n = 70: a second act workgroup with ragged rows and a second
    env-step block (64 envs per block); four policies of one agent each."""
    run_case(LOCAL, config, 3, n, 4)


@pytest.mark.parametrize("n", [20, 260])
def test_shared_three_members(n):
    """k = 4.  n = 20: 80 rows, the act workgroup boundary (64 rows) falls inside an env range.
    n = 260: two filter chunks, the second of 4 rows; five env-step blocks."""
    run_case(SHARED, None, 3, n, 3)


@pytest.mark.parametrize("env_name,config", [
    pytest.param(CUP_ENV, CUP_CONFIG, id="cup"),
    pytest.param(CENTRAL, None, id="centralized_A8"),
    pytest.param(TWOSIDES, None, id="twosides_A4"),
    pytest.param(CUP_ENV, None, id="legid_d23"),
])
def test_other_models(env_name, config):
    run_case(env_name, config, 2, 8, 3)


def test_episode_ends_inside_the_fragment():
    """TimeLimit 3 (+ m) with T = 8: every env restarts, each drawing its next target velocity from
    the member's own list (the TVel observation, D = 44, carries it into the policies)."""
    n, T, M = 8, 8, 3
    config = {"env_config": {"target_velocity": TVS}}
    dones = run_case("QuantrupedMultiEnv_FullyDecentral", config, M, n, T, limit=3, tvs=TVS)
    assert len(dones) == M
    for run, m, rows in dones:
        # the episode rows are {t, env, ...} of every done flag the fragment recorded
        assert set(rows[:, 1].astype(int)) == set(range(n)), (m, rows[:, 1])   # every env of every member ended
        assert n <= len(rows) < n * T, (m, len(rows))                          # ... and not at every step


@pytest.mark.parametrize("smooth", [None, 0.8], ids=["flat", "uneven"])
def test_per_env_target_velocities(smooth):
    """set_env_target_velocities on every member, each its own table: the per-env-velocity instances
    of the step kernel, flat and uneven.  n = 70 is two env-step blocks, so the table is read past
    env 63; TimeLimit 3 (+ m) with T = 8 restarts every env, which then holds its table entry."""
    n, T, M = 70, 8, 3
    config = {"env_config": {"target_velocity": TVS}}
    dones = run_case("QuantrupedMultiEnv_FullyDecentral", config, M, n, T, limit=3, tvs=TVS, smooth=smooth, tv_env=True)
    assert len(dones) == M
    for run, m, rows in dones:
        assert set(rows[:, 1].astype(int)) == set(range(n)), (m, rows[:, 1])   # every env of every member ended


def test_uneven_ground():
    """set_terrain 0.8: the terrain instance of the step kernel; each member its own bounds and generation."""
    run_case(LOCAL, None, 3, 8, 4, smooth=0.8, limit=3)


def test_two_runs_carry_state_and_honour_settings_between():
    """The second run (reset = 0) continues the first; new_terrain and set_time_limit between the
    runs reach the kernels through the rebuilt member table."""
    def between(env, m):
        env.new_terrain()
        env.set_time_limit(2 + m)
    dones = run_case(LOCAL, None, 2, 8, 4, runs=2, between=between, smooth=0.8)
    second = [rows for run, m, rows in dones if run == 1]
    assert all(len(rows) >= 8 for rows in second)          # the new time limit ended episodes


def test_one_member():
    run_case(LOCAL, PFILTER, 1, 70, 3)


def test_reset_run():
    """reset = 1 on contexts that have not stepped yet: ddrl_devenv_reset + observe for every member."""
    run_case(SHARED, PFILTER, 2, 20, 3, reset=True, warm=False)


# ---- refusals ---------------------------------------------------------------------------------
def _refused(contexts, envs, match):
    with pytest.raises(N.DdrlError, match=match):
        N.RolloutGroup(contexts, envs).close()


def test_refusals_have_messages():
    import ctypes as C
    import torch
    n, T = 8, 3
    a, b = Member(LOCAL, None, n, T, 0, warm=False), Member(LOCAL, None, n, T, 1, warm=False)
    lib = N.load()
    h = N.VP()
    with pytest.raises(N.DdrlError, match="at least one member"):
        N._ck(lib.ddrl_rollout_group_create((N.VP * 1)(), (N.VP * 1)(), 0, C.byref(h)))
    with pytest.raises(N.DdrlError, match="member 1 is a null context"):
        N._ck(lib.ddrl_rollout_group_create((N.VP * 2)(a.ctx.h, None), (N.VP * 2)(a.env.h, b.env.h), 2, C.byref(h)))
    with pytest.raises(N.DdrlError, match="member 1 has a null device env"):
        N._ck(lib.ddrl_rollout_group_create((N.VP * 2)(a.ctx.h, b.ctx.h), (N.VP * 2)(a.env.h, None), 2, C.byref(h)))
    _refused([a.ctx, a.ctx], [a.env, b.env], "member 1 repeats member 0")
    extra = N.DevEnv(b.ctx, seed=1)
    _refused([a.ctx, b.ctx], [a.env, a.env], "member 1 repeats the device env of member 0")
    _refused([a.ctx, b.ctx], [b.env, a.env], "member 0: its device env is bound to another context")
    N.RolloutGroup([a.ctx, b.ctx], [a.env, extra]).close()   # a second env of the member's own context is fine
    # shape: n_envs, frag_len, another env class, the per-policy filter
    for other, why in ((Member(LOCAL, None, n + 1, T, 1, warm=False), "n_envs"),
                       (Member(LOCAL, None, n, T + 1, 1, warm=False), "frag_len"),
                       (Member(SHARED, None, n, T, 1, warm=False), "n_policies"),
                       (Member(LOCAL, PFILTER, n, T, 1, warm=False), "policy_filter"),
                       (Member(LOCAL, {"env_config": {"contact_cost_weight": 1e-2}}, n, T, 1, warm=False),
                        "contact_cost_weight")):
        _refused([a.ctx, other.ctx], [a.env, other.env], f"member 1 differs from member 0 in {why}")
        other.close()
    g = Member(GNN_ENV, None, n, T, 1, warm=False, gnn=True)
    _refused([g.ctx], [g.env], "member 0 is a GraphNet context")
    _refused([a.ctx, g.ctx], [a.env, g.env], "member 1 is a GraphNet context")
    g.close()
    # another stream
    side = torch.cuda.Stream()
    b.ctx.set_stream(side.cuda_stream)
    _refused([a.ctx, b.ctx], [a.env, b.env], "member 1 is on another stream than member 0")
    b.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    # terrain on / off and the velocity mode, at create ...
    b.env.set_terrain(0.8)
    _refused([a.ctx, b.ctx], [a.env, b.env], "member 1 has its terrain on and member 0 off")
    b.env.set_terrain(1.0)
    b.env.set_env_target_velocities(np.ones(n, np.float32))
    _refused([a.ctx, b.ctx], [a.env, b.env], "member 1 and member 0 differ in the target-velocity mode")
    b.env.set_env_target_velocities(None)
    # ... and again at run; after a refusal the group still runs once the cause is gone, and closes
    group = N.RolloutGroup([a.ctx, b.ctx], [a.env, b.env])
    eps = [noise((T, n, a.cfg.n_agents, a.cfg.act_dim), m) for m in range(2)]
    b.env.set_terrain(0.8)
    with pytest.raises(N.DdrlError, match="member 1 has its terrain on and member 0 off"):
        group.run(eps)
    b.env.set_terrain(1.0)
    b.env.set_env_target_velocities(np.ones(n, np.float32))
    with pytest.raises(N.DdrlError, match="target-velocity mode"):
        group.run(eps)
    b.env.set_env_target_velocities(None)
    with pytest.raises(N.DdrlError, match="member 1: null noise buffer"):
        group.run([eps[0], None])
    with pytest.raises(N.DdrlError, match="2 noise buffers expected"):
        group.run(eps[:1])
    b.ctx.set_stream(side.cuda_stream)
    with pytest.raises(N.DdrlError, match="member 1 is on another stream"):
        group.run(eps)
    b.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(N.DdrlError, match="null rollout group"):
        N._ck(lib.ddrl_rollout_group_run(None, (N.VP * 2)(), 0))
    group.run(eps, reset=True)
    a.ctx.synchronize()
    assert np.isfinite(a.ctx.records_get(0)).all() and np.isfinite(b.ctx.records_get(0)).all()
    group.close()
    with pytest.raises(N.DdrlError, match="used after close"):
        group.run(eps)
    extra.close()
    a.close()
    b.close()
