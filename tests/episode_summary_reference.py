"""The per-row EpisodeHistory.summarize that ddrl_amd.metrics had before its rewrite on array
operations, kept verbatim as the reference of tests/test_episode_summary.py (pure Python over the
rows: one tuple and one inner list per finished episode)."""
import numpy as np


class EpisodeHistory:
    """The smoothing window of CollectMetrics: summarize(rows, ...) takes one iteration's
    finished episodes and returns RLlib's summary over the window."""

    def __init__(self, smoothing=100):
        self.smoothing = int(smoothing)
        self.history = []   # (total, length, [(policy index, agent total), ...]) per episode, oldest first

    @staticmethod
    def _episodes(rows, agent_policy):
        rows = np.asarray(rows, np.float64).reshape(-1, 8)
        agent_policy = [int(p) for p in agent_policy]
        return [(float(r[3]), int(r[2]), [(p, float(r[4 + j])) for j, p in enumerate(agent_policy)])
                for r in rows]

    def summarize(self, rows, agent_policy, policy_ids):
        """rows: [n, 8] in (t, env) order; agent_policy: policy index of every agent;
        policy_ids: the policies' names.  Returns the EPISODE_KEYS dict."""
        new = self._episodes(rows, agent_policy)
        episodes = list(new)
        missing = max(0, self.smoothing - len(episodes))
        if missing > 0:
            episodes = self.history[-missing:] + episodes
        self.history.extend(new)
        self.history = self.history[-self.smoothing:] if self.smoothing > 0 else []

        rewards = [ep[0] for ep in episodes]
        lengths = [ep[1] for ep in episodes]
        policy_rewards = {}
        for ep in episodes:
            for p, r in ep[2]:
                policy_rewards.setdefault(policy_ids[p], []).append(r)
        nan = float("nan")
        hist = {"episode_reward": rewards, "episode_lengths": lengths}
        pmin, pmax, pmean = {}, {}, {}
        for pid, rs in policy_rewards.items():
            pmin[pid] = float(np.min(rs))
            pmax[pid] = float(np.max(rs))
            pmean[pid] = float(np.mean(rs))
            hist[f"policy_{pid}_reward"] = rs
        return {
            "episode_reward_max": float(np.max(rewards)) if rewards else nan,
            "episode_reward_min": float(np.min(rewards)) if rewards else nan,
            "episode_reward_mean": float(np.mean(rewards)) if rewards else nan,
            "episode_len_mean": float(np.mean(lengths)) if lengths else nan,
            "episodes_this_iter": len(new),
            "policy_reward_min": pmin,
            "policy_reward_max": pmax,
            "policy_reward_mean": pmean,
            "custom_metrics": {},
            "hist_stats": hist,
            "sampler_perf": {},
            "off_policy_estimator": {},
        }
