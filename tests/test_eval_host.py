"""CPU checks of what evaluation needs from the host env plane (the pre-reset kin buffer, the
settable TimeLimit, reset_episodes), of the numpy evaluation reference against a hand-computed
case, and of the error paths of the ddrl_eval_* entry points that need no device.

Reference: evaluation/rollout_episodes.py:83 (episode length limit), :122, :146-151 (the
accumulated quantities)."""
import ctypes

import numpy as np
import pytest

from ddrl_amd import build, native as N
from tests import eval_reference as R


@pytest.fixture(scope="module")
def lib():
    build.build()
    return N.load()


def _run(env, steps, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        env.act[:] = rng.uniform(-1.2, 1.2, size=env.act.shape).astype(np.float32)
        env.step()
        out.append(dict(obs=env.obs.copy(), fw=env.fw.copy(), kin=env.kin.copy(), done=env.done.copy(),
                        act=env.act.copy()))
    return out


@pytest.mark.parametrize("D", [43, 44])
def test_kin_is_the_step_before_any_reset(lib, D):
    env = N.HostEnv(37, D, n_threads=2, seed=5, target_velocity=1.5 if D == 44 else 0.0)
    env.set_time_limit(25)   # with reset()'s staggered phases: episode ends on most of the 60 steps
    env.reset()
    assert env.kin.shape == (37, 9) and env.kin.dtype == np.float32
    n_done = n_live = 0
    for s in _run(env, 60, 11):
        live = s["done"] == 0
        n_live += int(live.sum())
        n_done += int((~live).sum())
        # joint velocities: the same doubles cast to fp32 as the observation's qvel[6:14]
        np.testing.assert_array_equal(s["kin"][live, 1:9], s["obs"][live, 19:27])
        if D == 43:   # fw = (float)(dx / 0.05), kin[0] = (float)dx
            np.testing.assert_allclose(s["kin"][:, 0], s["fw"].astype(np.float64) * 0.05, rtol=1e-6, atol=1e-9)
        if (~live).any():
            k, o = s["kin"][~live], s["obs"][~live]
            assert np.all(np.any(k[:, 1:9] != 0, axis=1))     # the episode's last joint velocities
            assert np.all(o[:, 35:43] == 0)                   # the reset observation: ctrl columns 0
            assert np.all(np.any(k[:, 1:9] != o[:, 19:27], axis=1))
    assert n_done >= 37 and n_live >= 37 * 30, (n_done, n_live)   # guards the input
    env.close()
    assert env.kin is None


def test_time_limit_and_reset_episodes(lib):
    runs = {}
    for threads in (1, 4):
        env = N.HostEnv(37, 43, n_threads=threads, seed=3)
        env.set_time_limit(7)
        obs0 = env.reset_episodes()
        assert not env.done.any() and np.all(obs0[:, 35:43] == 0)
        log = _run(env, 10, 17)
        done = np.stack([s["done"] for s in log])
        first = np.array([np.flatnonzero(done[:, e])[0] if done[:, e].any() else -1 for e in range(37)])
        assert np.all(first <= 6) and np.all(first >= 0)       # step 7 (index 6) at the latest
        assert int((first == 6).sum()) >= 30, first             # exactly at the limit unless unhealthy
        # mid-episode: a second reset_episodes starts new episodes at step 0
        obs1 = env.reset_episodes()
        assert not env.done.any()
        assert not np.array_equal(obs0, obs1)                   # new episodes, new initial poses
        log2 = _run(env, 7, 19)
        done2 = np.stack([s["done"] for s in log2])
        first2 = np.array([np.flatnonzero(done2[:, e])[0] if done2[:, e].any() else -1 for e in range(37)])
        assert np.all(first2 >= 0) and int((first2 == 6).sum()) >= 30, first2
        runs[threads] = log + log2
        env.close()
    for a, b in zip(runs[1], runs[4]):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_set_time_limit_rejects_bad_values(lib):
    env = N.HostEnv(2, 43)
    with pytest.raises(N.DdrlError, match="steps >= 1"):
        env.set_time_limit(0)
    env.close()


def test_reference_accumulator_hand_computed():
    """2 envs, 5 steps, E = 2.  env 0: an episode of length 1, then one of length 4.  env 1: a
    zero-distance episode of length 3 (velocity 0, CoT inf), then two steps without an end."""
    m = R.TOTAL_MASS
    acc = R.EpisodeAccumulator(2, 2)
    rewards = [[1.5, -1.0], [1.0, -1.0], [2.0, -1.0], [3.0, 7.0], [4.0, 7.0]]
    done = [[1, 0], [0, 0], [0, 1], [0, 0], [1, 0]]
    for t in range(5):
        actions = np.zeros((2, 8), np.float32)
        kin = np.zeros((2, 9), np.float32)
        # np.roll(ctrl, -2)[j] = ctrl[(j + 2) % 8]: env 0 pairs ctrl[0] with qvel[6], env 1 ctrl[2] with qvel[0]
        actions[0, 0] = 0.5 if t == 0 else -0.25
        kin[0, 1 + 6] = 2.0
        kin[0, 0] = 0.25 if t == 0 else 0.5
        actions[1, 2] = 1.0
        kin[1, 1 + 0] = 2.0
        acc.step(rewards[t], actions, kin, done[t])
    want = np.array([[[1.5, 1, 0.25, 1.0, 0.25, (1.0 / 1) / (m * 0.25)],
                      [10.0, 4, 2.0, 2.0, 0.5, (2.0 / 4) / (m * 0.5)]],
                     [[-3.0, 3, 0.0, 6.0, 0.0, np.inf],
                      [np.nan] * 6]])
    np.testing.assert_array_equal(acc.table, want)
    assert acc.episodes_done == 3 and acc.envs_finished == 1


def test_eval_entry_points_report_null_arguments(lib):
    """No device call is reached: a null context or host env is refused with a message."""
    z = ctypes.c_int64()
    ec = N.DdrlEvalCfg(1, 0, 2, 0, N.TOTAL_MASS)
    calls = [lambda: lib.ddrl_eval_begin(None, ctypes.byref(ec)),
             lambda: lib.ddrl_eval_act(None, None, None, None, None),
             lambda: lib.ddrl_eval_step(None, None, None, None, None, None),
             lambda: lib.ddrl_eval_progress(None, ctypes.byref(z), ctypes.byref(z)),
             lambda: lib.ddrl_eval_results(None, None, 0),
             lambda: lib.ddrl_eval_end(None),
             lambda: lib.ddrl_eval_hostenv(None, None, None, 0, 1, 1, None)]
    for call in calls:
        assert call() != 0
        assert b"null context" in lib.ddrl_last_error()
    for call in (lambda: lib.ddrl_hostenv_kin(None, None), lambda: lib.ddrl_hostenv_set_time_limit(None, 5),
                 lambda: lib.ddrl_hostenv_reset_episodes(None)):
        assert call() != 0
        assert b"null" in lib.ddrl_hostenv_last_error() or b"host env" in lib.ddrl_hostenv_last_error()
    assert ctypes.sizeof(N.DdrlEvalCfg) == 24 and N.DdrlEvalCfg.total_mass.offset == 16
