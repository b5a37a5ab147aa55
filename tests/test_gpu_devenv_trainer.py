"""PPOTrainer over the device env plane: config["env_backend"] = "device" trains with the envs
stepped by a kernel on the rollout context's stream, and evaluate(..., env_backend="device") runs
ddrl_eval_devenv; the default evaluation backend stays the host plane."""
import numpy as np
import pytest

from ddrl_amd import native as N

pytestmark = pytest.mark.gpu
N_ENVS, T = 8, 16
CFG = {"env": "QuantrupedMultiEnv_Local", "rollout_fragment_length": T, "env_backend": "device"}


def _check_tuple(res, n, num_steps):
    assert len(res) == 6 and all(isinstance(col, list) and len(col) == n for col in res)
    reward, steps, dist, power, vel, cot = (np.asarray(c, np.float64) for c in res)
    for col in (reward, steps, dist, power, vel):
        assert np.isfinite(col).all()
    assert all(isinstance(s, int) for s in res[1]) and steps.min() >= 1 and steps.max() <= num_steps
    np.testing.assert_array_equal(vel, dist / steps)
    with np.errstate(divide="ignore", invalid="ignore"):   # CoT where distance is 0: as the host path defines
        np.testing.assert_array_equal(cot, (power / steps) / (N.TOTAL_MASS * vel))
    assert np.isfinite(cot[dist != 0]).all() and (power > 0).all()


def test_training_over_the_device_env_plane():
    from ddrl_amd.envs import DeviceVecEnv
    from ddrl_amd.trainer import PPOTrainer
    tr = PPOTrainer(CFG, n_envs=N_ENVS, seed=3)
    assert isinstance(tr.backend, DeviceVecEnv) and tr.backend.env.ctx is tr.rctx
    tr.backend.env.set_time_limit(10)      # short episodes: every fragment ends some
    dones, step = [], tr.backend.step

    def recording_step(actions):
        out = step(actions)
        assert all(x.is_cuda for x in out)                # device tensors, the plane's own buffers
        assert out[0].data_ptr() == tr.backend.env.obs.data_ptr()
        dones.append(out[3].cpu().numpy().copy())
        return out
    tr.backend.step = recording_step
    total = 0
    for it in range(2):
        r = tr.train()
        done = np.stack(dones[it * T:(it + 1) * T])
        assert r["episodes_this_iter"] == int(done.sum()) > 0
        total += int(done.sum())
        assert r["episodes_total"] == total and r["timesteps_total"] == (it + 1) * T * N_ENVS
        assert np.isfinite(r["episode_reward_mean"]) and 1 <= r["episode_len_mean"] <= 10
        for pid, st in r["info"]["learner"].items():
            for k, v in st.items():
                assert np.isfinite(v), (pid, k)
    tr.workers.foreach_worker(lambda w: w.foreach_env(lambda env: env.update_environment_after_epoch(0)))
    assert (tr.backend.env.state()[:, N.ENV_STATE_COLUMNS["steps"]] == 0).all()
    tr.stop()


def test_tvel_lists_reach_the_device_backend():
    from ddrl_amd.trainer import PPOTrainer
    tvs = [0.5, 1.0, 2.0]
    tr = PPOTrainer({**CFG, "env_config": {"target_velocity": tvs}}, n_envs=64, seed=1)
    got = tr.backend.target_velocities
    assert set(np.unique(got)) == set(np.float32(tvs))
    np.testing.assert_array_equal(tr.backend.env.obs[:, 43].cpu().numpy(), got)
    tr.stop()


def test_evaluate_on_the_device_plane_and_the_default_stays_host(monkeypatch):
    from ddrl_amd.trainer import PPOTrainer
    tr = PPOTrainer(CFG, n_envs=N_ENVS, seed=3)
    made = {"host": 0, "device": 0}
    host_init, dev_init = N.HostEnv.__init__, N.DevEnv.__init__

    def count(kind, init):
        def wrapped(self, *a, **k):
            made[kind] += 1
            init(self, *a, **k)
        return wrapped
    monkeypatch.setattr(N.HostEnv, "__init__", count("host", host_init))
    monkeypatch.setattr(N.DevEnv, "__init__", count("device", dev_init))
    args = dict(num_episodes=12, num_steps=20, explore=False, env_filter="frozen")
    res = tr.evaluate(env_backend="device", **args)
    assert made == {"host": 0, "device": 1}
    _check_tuple(res, 12, 20)
    assert tr.evaluate(env_backend="device", **args) == res      # frozen filter, same seed: the same lists
    ectx = tr._eval_context(12)
    assert ectx.cfg.n_envs == 12                                  # 12 envs, one episode each: no 128 cap in play
    # more episodes than the host path's 128 envs: one episode per env
    many = tr.evaluate(num_episodes=200, num_steps=20, env_backend="device")
    _check_tuple(many, 200, 20)
    assert tr._eval_context(200).cfg.n_envs == 200
    sens_lists, sens = tr.evaluate_sensitivity(num_episodes=12, num_steps=20, env_backend="device", **{
        k: v for k, v in args.items() if k not in ("num_episodes", "num_steps")})
    assert sens_lists == res and all(s["rows"] > 0 for s in sens.values())
    made.update(host=0, device=0)
    host = tr.evaluate(**args)                                    # the default backend: the host plane
    assert made == {"host": 1, "device": 0}
    _check_tuple(host, 12, 20)
    assert host[1] == res[1]                                      # the same episode lengths on either plane
    with pytest.raises(ValueError, match="env_backend"):
        tr.evaluate(env_backend="other")
    tr.stop()
