"""PPOTrainer.train() reports RLlib's episode keys (episode_reward_mean & co.) from the on-device
episode accounting, and run(..., logdir=...) writes Tune's progress.csv / result.json.

The numbers are checked against tests/episodes_reference.py run on the trainer's own records (the
fp32 rewards of every fragment and the done flags its env backend raised) and
ddrl_amd.metrics.EpisodeHistory's window over them: exact equality, there is no tolerance."""
import csv
import json
import math

import numpy as np
import pytest

from ddrl_amd.metrics import EPISODE_KEYS, EpisodeHistory
from tests import episodes_reference as R

pytestmark = pytest.mark.gpu
N_ENVS, T = 8, 16
TRAINER_KEYS = ["num_healthy_workers", "timesteps_total", "timers", "info", "done", "episodes_total",
                "training_iteration"]


class _RecordingEnv:
    """The synthetic backend with short episodes, keeping the done flags it raised."""

    def __init__(self, obs_dim, device, seed):
        from ddrl_amd.envs import SyntheticVecEnv
        self.env = SyntheticVecEnv(N_ENVS, obs_dim, device, seed=seed, max_episode_steps=20)
        self.dones = []

    def reset(self):
        return self.env.reset()

    def step(self, actions):
        out = self.env.step(actions)
        self.dones.append(out[3].cpu().numpy().copy())
        return out


def _trainer(env, parallel=None, seed=3):
    import torch
    from ddrl_amd.spec import make_cfg
    from ddrl_amd.trainer import PPOTrainer
    cfg, _ = make_cfg(env, N_ENVS, T)
    backend = _RecordingEnv(cfg.obs_full_dim, torch.device("cuda", 0), seed)
    config = {"env": env, "rollout_fragment_length": T}
    if parallel:
        config["parallel"] = parallel
    return PPOTrainer(config, n_envs=N_ENVS, env_backend=backend, seed=seed), backend


def _train_and_check(tr, backend, iters=3):
    ref = R.EpisodeReference(N_ENVS, tr.cfg.n_agents)
    hist = EpisodeHistory(100)
    agent_policy = [p for p, _ in R.agent_slots(tr.cfg)]
    results, total = [], 0
    for it in range(iters):
        r = tr.train()
        done = np.stack(backend.dones[it * T:(it + 1) * T])
        rows = ref.fragment(R.record_rewards(tr.rctx, tr.cfg), done)
        want = hist.summarize(rows, agent_policy, tr.policy_ids)
        total += rows.shape[0]
        keys = list(r)
        assert keys[:len(EPISODE_KEYS)] == list(EPISODE_KEYS)
        assert keys[len(EPISODE_KEYS):len(EPISODE_KEYS) + len(TRAINER_KEYS)] == TRAINER_KEYS
        assert r["episodes_this_iter"] == rows.shape[0] == int(done.sum())
        assert r["hist_stats"] == want["hist_stats"]
        for k in EPISODE_KEYS:
            if isinstance(want[k], float) and math.isnan(want[k]):
                assert math.isnan(r[k]), k
            else:
                assert r[k] == want[k], k
        assert r["episodes_total"] == total and r["num_healthy_workers"] == 1 and r["custom_metrics"] == {}
        assert r["training_iteration"] == it + 1 and r["timesteps_total"] == (it + 1) * T * N_ENVS
        results.append(r)
    np.testing.assert_array_equal(tr.rctx.episodes_inflight(), ref.inflight())
    assert total > 0
    return results


@pytest.mark.parametrize("env", ["QuantrupedMultiEnv_Local", "QuantrupedMultiEnv_SharedDecentral"])
def test_train_reports_the_episode_keys(env):
    seen = []
    config_cb = {"on_train_result": lambda info: seen.append(info["result"]["episode_reward_mean"])}
    tr, backend = _trainer(env)
    tr.config["callbacks"] = config_cb
    results = _train_and_check(tr, backend)
    assert len(seen) == 3                                              # the callback sees the keys
    for s, r in zip(seen, results):
        assert s == r["episode_reward_mean"] or (math.isnan(s) and math.isnan(r["episode_reward_mean"]))
    last = results[-1]
    assert set(last["policy_reward_mean"]) == set(tr.policy_ids)
    per_episode = 4 if env.endswith("SharedDecentral") else 1
    n = len(last["hist_stats"]["episode_reward"])
    assert len(last["hist_stats"][f"policy_{tr.policy_ids[0]}_reward"]) == per_episode * n
    tr.stop()


def test_gather_mode_reports_what_replicas_reports():
    env = "QuantrupedMultiEnv_Local"
    ta, ba = _trainer(env)
    tb, bb = _trainer(env, parallel="gather")
    assert tb.rctx is not tb.ctx
    ra, rb = _train_and_check(ta, ba), _train_and_check(tb, bb)
    # the same seeds: the same first fragment, and the same done flags throughout
    for k in EPISODE_KEYS:
        a, b = ra[0][k], rb[0][k]
        assert a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b)), k
    assert [r["episodes_this_iter"] for r in ra] == [r["episodes_this_iter"] for r in rb]
    assert [r["episodes_total"] for r in ra] == [r["episodes_total"] for r in rb]
    ta.stop()
    tb.stop()


def test_run_stops_on_the_reward_mean_and_writes_progress(tmp_path):
    from ddrl_amd.trainer import run
    logdir = tmp_path / "trial"
    results = run({"env": "QuantrupedMultiEnv_Local", "rollout_fragment_length": T},
                  stop={"episode_reward_mean": -1e30}, n_envs=N_ENVS, verbose=False, logdir=str(logdir))
    # a nan mean never stops; the first iteration with an episode does
    assert all(r["episodes_this_iter"] == 0 and math.isnan(r["episode_reward_mean"]) for r in results[:-1])
    assert results[-1]["episodes_this_iter"] >= 1 and math.isfinite(results[-1]["episode_reward_mean"])
    with open(logdir / "progress.csv", newline="") as fh:
        lines = list(csv.reader(fh))
    assert lines[0][2] == "episode_reward_mean" and lines[0][6] == "timesteps_total"
    assert lines[0][:7] == ["episode_reward_max", "episode_reward_min", "episode_reward_mean", "episode_len_mean",
                            "episodes_this_iter", "num_healthy_workers", "timesteps_total"]
    assert len(lines) == len(results) + 1
    for ln, r in zip(lines[1:], results):
        assert int(ln[6]) == r["timesteps_total"]
        assert float(ln[2]) == r["episode_reward_mean"] or math.isnan(r["episode_reward_mean"])
    with open(logdir / "result.json") as fh:
        back = [json.loads(ln) for ln in fh]
    assert len(back) == len(results)
    assert back[-1]["hist_stats"] == results[-1]["hist_stats"]
    assert back[-1]["episode_reward_mean"] == results[-1]["episode_reward_mean"]
