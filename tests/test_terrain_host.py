"""Uneven ground on the host env plane, on the CPU: the probe (ddrl_hostenv_terrain_height) against
the numpy restatement of the field (tests/terrain_reference.py) bit for bit, the field's properties,
flat equivalence (an env told the ground is flat is byte-identical to one that never heard of
terrain), terrain acting on the feet and the torso but not on the joints, the settings round trip
and its refusals, and the update_environment_after_epoch hook with the reference's curriculum."""
import numpy as np
import pytest

from ddrl_amd import build, native as N
from ddrl_amd.envs import HostVecEnv, curriculum_bounds
from ddrl_amd.hostenv import HostMultiAgentEnv
from tests import terrain_reference as R

SEED, NENV = 43, 65
PTS = R.probe_points()
C = N.ENV_STATE_COLUMNS


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build()
    return N.load()


@pytest.fixture(scope="module")
def env():
    e = N.HostEnv(NENV, 43, 3, SEED)
    yield e
    e.close()


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _actions(n, t, seed=43):
    return np.random.default_rng(seed * 1000 + t).uniform(-1, 1, (n, 8)).astype(np.float32)


def _outputs(env):
    return [b.tobytes() for b in (env.obs, env.fw, env.cfrc, env.kin, env.done)]


@pytest.mark.parametrize("lo,hi", [(0.0, 0.0), (0.6, 0.6), (1.0, 1.0), (0.6, 1.0)])
def test_probe_matches_the_reference_bit_for_bit(env, lo, hi):
    assert len(PTS) >= 200 and (PTS < 0).any()
    episodes = env.state()[:, C["episode"]]
    for gen in (0, 7):
        env.set_terrain(lo, hi, 2.0, gen)
        for e in (0, 64):
            h = env.terrain_height(e, PTS)
            ref = R.heights(SEED, e, lo, hi, 2.0, gen, episodes, PTS)
            np.testing.assert_array_equal(_bits(h), _bits(ref))
            assert (h >= 0.0).all() and (h <= 1.0 - lo).all()
            patch = np.abs(PTS).max(1) <= 0.8
            assert patch.sum() >= 16 and (_bits(h[patch]) == 0).all()       # exactly +0.0 on the start patch
            if hi == 1.0 and lo == 1.0:
                assert (_bits(h) == 0).all()                                # s = 1 is identically 0.0
            else:
                assert (h[np.abs(PTS).max(1) > 3.0] > 0.0).mean() > 0.95
            s = R.smoothness(SEED, e, lo, hi, gen)
            assert lo <= s <= hi
    if lo < hi:     # the per-env draws differ, and lie strictly inside the range for these envs
        draws = [R.smoothness(SEED, e, lo, hi, 7) for e in range(NENV)]
        assert len(set(draws)) == NENV and lo < min(draws) and max(draws) < hi


def test_probe_another_bump_scale_and_episode(env):
    """A bump spacing that is no power of two, and envs that are in a later episode: the field is
    keyed by the env's episode number, so a reset gives an env new ground."""
    e2 = N.HostEnv(4, 43, 1, SEED)
    e2.set_terrain(0.3, 0.3, 1.7, 2)
    pts = np.concatenate([R.probe_points(1.7), PTS[:40]])
    before = e2.terrain_height(1, pts)
    np.testing.assert_array_equal(_bits(before), _bits(R.heights(SEED, 1, 0.3, 0.3, 1.7, 2, np.zeros(4), pts)))
    e2.reset()
    ep = e2.state()[:, C["episode"]]
    assert (ep == 1).all()
    after = e2.terrain_height(1, pts)
    np.testing.assert_array_equal(_bits(after), _bits(R.heights(SEED, 1, 0.3, 0.3, 1.7, 2, ep, pts)))
    assert not np.array_equal(before, after)
    e2.close()


def test_field_is_continuous_across_cell_boundaries(env):
    env.set_terrain(0.0, 0.0, 2.0, 1)
    rng = np.random.default_rng(5)
    worst = 0.0
    for b in (-12.0, -2.0, 4.0, 18.0, 30.0):                # cell boundaries at bump_scale 2.0, off the ramp
        other = rng.uniform(5.0, 30.0, 32)
        for axis in (0, 1):
            below, at, above = (np.stack([np.full(32, v), other] if axis == 0 else [other, np.full(32, v)], 1)
                                for v in (np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf)))
            hb, ha, hu = (env.terrain_height(3, p) for p in (below, at, above))
            worst = max(worst, np.abs(hb - ha).max(), np.abs(hu - ha).max())
    # one ulp of x moves the smoothstep weight by <= 1.5 ulp(x) / bump_scale, the height by less
    # than that times the lattice range (1): rounding level, where a discontinuous field would
    # jump by a lattice difference (~0.3)
    assert worst < 1e-13


def test_generation_env_and_threads(env):
    env.set_terrain(0.6, 0.6, 2.0, 0)
    far = PTS[np.abs(PTS).max(1) > 3.0]
    h0 = env.terrain_height(0, far)
    assert not np.array_equal(h0, env.terrain_height(1, far))       # another env: another field
    env.new_terrain()
    assert env.terrain["generation"] == 1
    h1 = env.terrain_height(0, far)
    assert not np.array_equal(h0, h1)                               # another generation: another field
    env.set_terrain(0.6, 0.6, 2.0, 0)
    np.testing.assert_array_equal(_bits(env.terrain_height(0, far)), _bits(h0))   # the same key: the same bits
    one = N.HostEnv(NENV, 43, 1, SEED)                              # ... whatever the thread count
    one.set_terrain(0.6)
    np.testing.assert_array_equal(_bits(one.terrain_height(0, far)), _bits(h0))
    idx = np.arange(len(far)) % NENV
    np.testing.assert_array_equal(_bits(one.terrain_height(idx, far)), _bits(env.terrain_height(idx, far)))
    one.close()


@pytest.mark.parametrize("D,tv", [(43, 0.0), (44, [0.5, 1.0, 2.0])])
def test_flat_terrain_is_the_flat_env_byte_for_byte(D, tv):
    n = 9
    a = N.HostEnv(n, D, 2, SEED, tv)             # never heard of terrain
    b = N.HostEnv(n, D, 2, SEED, tv)
    b.set_terrain(1, 1)
    for _ in range(3):
        b.new_terrain()
    for e in (a, b):
        e.set_time_limit(15)
        e.reset()
    for t in range(40):
        for e in (a, b):
            e.act[:] = _actions(n, t)
            e.step()
        assert _outputs(a) == _outputs(b), t
        np.testing.assert_array_equal(_bits(a.state()), _bits(b.state()))
    a.close()
    b.close()


def _at_x10(n, D, tv, smooth):
    """An env plane a few steps into its episodes, moved to x = 10 m (past the start patch's ramp)."""
    e = N.HostEnv(n, D, 2, SEED, tv)
    e.reset()
    for t in range(6):
        e.act[:] = _actions(n, t)
        e.step()
    s = e.state()
    s[:, 0] = 10.0
    s[:, 1] = np.linspace(-3.0, 3.0, n)
    e.set_state(s)
    if smooth is not None:
        e.set_terrain(smooth)
    return e


@pytest.mark.parametrize("D,tv", [(43, 0.0), (44, 1.0)])
def test_terrain_acts_on_feet_and_torso_not_on_joints(D, tv):
    n = 8
    flat, rough = _at_x10(n, D, tv, None), _at_x10(n, D, tv, 0.6)
    np.testing.assert_array_equal(_bits(flat.state()), _bits(rough.state()))
    for t in range(6, 12):           # the feet of some envs are in the air for a step or two
        for e in (flat, rough):
            e.act[:] = _actions(n, t)
            e.step()
        sf, sr = flat.state(), rough.state()
        # the stand-in's joints do not feel the ground
        for col in ("q", "qd", "qfrc"):
            np.testing.assert_array_equal(_bits(sf[:, C[col]]), _bits(sr[:, C[col]]))
        if t == 6:
            first_foot = (sf[:, C["foot"]] != sr[:, C["foot"]]).any(1)
            first_torso = (sf[:, C["torso"]] != sr[:, C["torso"]]).any(1)
            first_tilt = (sf[:, 6:10] != sr[:, 6:10]).any(1)        # roll, pitch and their rates
            assert not np.array_equal(flat.cfrc, rough.cfrc)        # the forces reach cfrc
    assert first_foot.all() and first_torso.all()                   # after one step, in every env
    assert first_tilt.all()                                         # feet on differing ground: uneven torque
    flat.close()
    rough.close()


def test_settings_round_trip_and_refusals():
    e = N.HostEnv(3, 43)
    assert e.terrain == {"lo": 1.0, "hi": 1.0, "bump_scale": 2.0, "generation": 0}
    e.set_terrain(0.25, 0.75, 1.5, 9)
    e.new_terrain()
    assert e.terrain == {"lo": 0.25, "hi": 0.75, "bump_scale": 1.5, "generation": 10}
    e.set_terrain(0.5)                                               # hi None: fixed; generation kept
    assert e.terrain == {"lo": 0.5, "hi": 0.5, "bump_scale": 2.0, "generation": 10}
    for args, msg in (((0.8, 0.6), "lo <= hi"), ((0.5, 1.5), "hi <= 1"), ((-0.1, 0.5), "0 <= lo"),
                      ((float("nan"), 1.0), "0 <= lo"), ((0.5, 0.5, 0.0), "bump_scale"), ((0.5, 0.5, -2.0), "bump_scale")):
        with pytest.raises(N.DdrlError, match=msg):
            e.set_terrain(*args)
    assert e.terrain == {"lo": 0.5, "hi": 0.5, "bump_scale": 2.0, "generation": 10}   # a refusal changes nothing
    with pytest.raises(N.DdrlError, match="out of range"):
        e.terrain_height(3, [[0.0, 0.0]])
    assert e.terrain_height(0, np.zeros((0, 2))).shape == (0,)
    e.close()
    for call in (lambda: e.set_terrain(0.5), lambda: e.terrain, e.new_terrain, lambda: e.terrain_height(0, [[1.0, 1.0]])):
        with pytest.raises(N.DdrlError, match="closed"):
            call()


def test_curriculum_bounds_are_the_adaptors():
    # adaptor :104-120 with range_smoothness [1.0, 0.6]: rand() in [0, 1) scales the distance from the
    # initial smoothness, so the draws span (lo, hi] with these bounds
    assert curriculum_bounds(1.0, 0.6, 1000, 0) == (1.0, 1.0)
    lo, hi = curriculum_bounds(1.0, 0.6, 1000, 500)
    assert hi == 1.0 and lo == 1.0 - (1.0 - 0.6) * 0.5
    assert curriculum_bounds(1.0, 0.6, 1000, 1000) == (0.6, 1.0)
    assert curriculum_bounds(1.0, 0.6, 1000, 5000) == (0.6, 1.0)


CURRICULUM = {"curriculum_learning": True, "range_smoothness": [1.0, 0.6], "range_last_timestep": 1000}


def _moved(env_plane, n):
    env_plane.reset()
    for t in range(3):
        env_plane.act[:] = _actions(n, t)
        env_plane.step()
    return env_plane.state()


def _check_reset_state(before, after):
    """reset_state as before terrain: a fresh pose at step 0 of the next episode, velocity kept."""
    assert (after[:, C["steps"]] == 0).all()
    np.testing.assert_array_equal(after[:, C["episode"]], before[:, C["episode"]] + 1)
    np.testing.assert_array_equal(after[:, C["tv"]], before[:, C["tv"]])
    assert (after[:, 0] == 0).all() and (np.abs(after[:, 2] - 0.57) <= 0.01).all()


def test_backend_hook_and_curriculum():
    n = 5
    be = HostVecEnv.__new__(HostVecEnv)         # the backend without a device: only the hook is under test
    be.env = N.HostEnv(n, 43, 1, SEED)
    be.env.set_terrain(0.8)
    be.curriculum = (1.0, 0.6, 1000.0)
    for k, (ts, want) in enumerate([(0, (1.0, 1.0)), (500, (0.8, 1.0)), (2000, (0.6, 1.0))]):
        before = _moved(be.env, n)
        be.update_environment_after_epoch(ts)
        t = be.terrain
        assert (t["lo"], t["hi"]) == pytest.approx(want, abs=1e-15) and t["generation"] == k + 1
        _check_reset_state(before, be.env.state())
    be.curriculum = None                         # without curriculum_learning only the generation moves
    before = _moved(be.env, n)
    be.update_environment_after_epoch(123)
    assert be.terrain == {"lo": 0.6, "hi": 1.0, "bump_scale": 2.0, "generation": 4}
    _check_reset_state(before, be.env.state())
    be.close()


def test_dict_api_hook_and_reference_names():
    m = HostMultiAgentEnv("QuantrupedMultiEnv_Local", {"hf_smoothness": 0.8, **CURRICULUM}, n_envs=4, seed=SEED)
    assert m.terrain == {"lo": 0.8, "hi": 0.8, "bump_scale": 2.0, "generation": 0}
    for k, (ts, want) in enumerate([(0, (1.0, 1.0)), (500, (0.8, 1.0)), (1500, (0.6, 1.0))]):
        before = _moved(m.env, 4)
        m.update_environment_after_epoch(ts)
        assert (m.terrain["lo"], m.terrain["hi"]) == pytest.approx(want, abs=1e-15) and m.terrain["generation"] == k + 1
        _check_reset_state(before, m.env.state())
    m.close()
    m = HostMultiAgentEnv("QuantrupedMultiEnv_Local", {"hf_smoothness": 0.7}, n_envs=2, seed=SEED)
    before = _moved(m.env, 2)
    m.update_environment_after_epoch(10)        # no curriculum: only the generation moves
    assert m.terrain == {"lo": 0.7, "hi": 0.7, "bump_scale": 2.0, "generation": 1}
    _check_reset_state(before, m.env.state())
    m.create_new_random_hfield()
    m.set_hf_parameter(0.4)
    assert m.terrain == {"lo": 0.4, "hi": 0.4, "bump_scale": 2.0, "generation": 2}
    m.set_hf_parameter(0.3, bump_scale=1.0)
    assert m.terrain == {"lo": 0.3, "hi": 0.3, "bump_scale": 1.0, "generation": 2}
    far = [[12.0, 3.0], [-9.0, 4.5]]
    assert (m.env.terrain_height(0, far) > 0).all()
    m.close()
    with pytest.raises(ValueError, match="range_smoothness"):
        HostMultiAgentEnv("QuantrupedMultiEnv_Local", {"curriculum_learning": True}, n_envs=1)
