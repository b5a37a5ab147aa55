"""The host env plane's packed-state accessors (ddrl_hostenv_state_get / _set), on the CPU: the
layout's width is the header's constant, a state read back and written again changes nothing,
and an env restored from another's state mid-episode continues with byte-identical outputs."""
import re

import numpy as np
import pytest

from ddrl_amd import build, native as N


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build()
    return N.load()


def _actions(n, t, seed=43):
    return np.random.default_rng(seed * 1000 + t).uniform(-1, 1, (n, 8)).astype(np.float32)


def _outputs(env):
    return [b.tobytes() for b in (env.obs, env.fw, env.cfrc, env.kin, env.done)]


def test_layout_width_matches_the_header():
    txt = open(N.HEADER).read()
    width = int(re.search(r"#define\s+DDRL_ENV_STATE_DOUBLES\s+(\d+)", txt).group(1))
    assert width == N.ENV_STATE_DOUBLES == 10 + 8 + 8 + 8 + 4 + 3
    cols = N.ENV_STATE_COLUMNS
    flat = np.arange(width)
    covered = np.concatenate([np.atleast_1d(flat[c]) for c in cols.values()])
    np.testing.assert_array_equal(np.sort(covered), flat)   # every column named once
    env = N.HostEnv(3, 43)
    assert env.state().shape == (3, width) and env.state().dtype == np.float64
    env.close()


@pytest.mark.parametrize("D,tv", [(43, 0.0), (44, [0.5, 1.0, 2.0])])
def test_state_round_trip_and_columns(D, tv):
    n = 9
    env = N.HostEnv(n, D, 2, 43, tv)
    env.set_time_limit(20)
    env.reset()
    for t in range(7):
        env.act[:] = _actions(n, t)
        env.step()
    s = env.state()
    c = N.ENV_STATE_COLUMNS
    # the columns are what the env's own outputs show of the state
    np.testing.assert_array_equal(s[:, c["q"]].astype(np.float32), env.obs[:, 5:13])
    np.testing.assert_array_equal(s[:, c["qd"]].astype(np.float32), env.obs[:, 19:27])
    np.testing.assert_array_equal(s[:, c["qfrc"]].astype(np.float32), env.obs[:, 27:35])
    np.testing.assert_array_equal(s[:, 2].astype(np.float32), env.obs[:, 0])          # torso z
    np.testing.assert_array_equal(s[:, 3:6].astype(np.float32), env.obs[:, 13:16])    # vx, vy, vz
    np.testing.assert_array_equal(s[:, c["tv"]].astype(np.float32), env.target_velocities)
    assert (s[:, c["steps"]] >= 0).all() and (s[:, c["steps"]] < 20).all() and (s[:, c["episode"]] >= 1).all()
    before = _outputs(env)
    env.set_state(s)
    np.testing.assert_array_equal(env.state().view(np.uint64), s.view(np.uint64))
    assert _outputs(env) == before            # set_state leaves the output buffers alone
    with pytest.raises(N.DdrlError, match="DDRL_ENV_STATE_DOUBLES"):
        env.set_state(s[:-1])
    bad = s.copy()
    bad[0, c["steps"]] = -1.0
    with pytest.raises(N.DdrlError, match="non-negative integers"):
        env.set_state(bad)
    env.close()
    with pytest.raises(N.DdrlError, match="closed"):
        env.state()


@pytest.mark.parametrize("D,tv", [(43, 0.0), (44, [0.5, 1.0, 2.0])])
def test_restored_env_continues_byte_identically(D, tv):
    n = 16
    a = N.HostEnv(n, D, 2, 43, tv)
    b = N.HostEnv(n, D, 1, 43, tv)     # same seed: the same reset draws at the same episode numbers
    for env in (a, b):
        env.set_time_limit(20)
    a.reset()
    for t in range(13):                # mid-episode for most envs, some already in a later episode
        a.act[:] = _actions(n, t)
        a.step()
    assert not np.array_equal(a.state(), b.state())
    b.set_state(a.state())
    ends = 0
    for t in range(13, 63):
        for env in (a, b):
            env.act[:] = _actions(n, t)
            env.step()
        assert _outputs(a) == _outputs(b), t
        ends += int(a.done.sum())
    assert ends >= n                   # the 50 steps cross episode ends (resets and new draws) in every env
    np.testing.assert_array_equal(a.state().view(np.uint64), b.state().view(np.uint64))
    a.close()
    b.close()
