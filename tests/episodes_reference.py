"""Plain-Python restatement of RLlib 1.0's episode accounting, for the episode tests.

3p evaluation/episode.py MultiAgentEpisode._add_agent_rewards: for every env step, for every agent
in agent order, agent_rewards[(agent, policy)] += r and total_reward += r (Python floats, fp64);
length counts env steps; the step that raises done belongs to the episode it ends.  The loop runs
over (t, env, agent), so the finished episodes come out in ascending (t, env) order; the state of
the running episodes persists across fragments.
"""
import numpy as np


class EpisodeReference:
    def __init__(self, n_envs, n_agents):
        self.N, self.na = n_envs, n_agents
        self.reset()

    def reset(self):
        self.total = [0.0] * self.N
        self.agent = [[0.0] * 4 for _ in range(self.N)]
        self.length = [0] * self.N

    def fragment(self, rew, done):
        """rew: [T, N, n_agents] float32 rewards (the records' rew column), done: [T, N].
        Returns float64 [n, 8] rows {t, env, length, total, agent_0 .. agent_3} (NaN: no agent)."""
        T = rew.shape[0]
        rows = []
        for t in range(T):
            for e in range(self.N):
                for j in range(self.na):
                    r = float(rew[t, e, j])
                    self.agent[e][j] += r
                    self.total[e] += r
                self.length[e] += 1
                if done[t, e]:
                    rows.append([float(t), float(e), float(self.length[e]), self.total[e]] +
                                [self.agent[e][j] if j < self.na else float("nan") for j in range(4)])
                    self.total[e] = 0.0
                    self.agent[e] = [0.0] * 4
                    self.length[e] = 0
        return np.array(rows, np.float64).reshape(-1, 8)

    def inflight(self):
        """float64 [N, 6]: {total, agent_0 .. agent_3, length} of every env's running episode."""
        return np.array([[self.total[e]] + self.agent[e] + [float(self.length[e])] for e in range(self.N)],
                        np.float64).reshape(self.N, 6)


def agent_slots(cfg):
    """(policy, slot) of every agent: agent j of env e is record row e * k_p + slot of policy p."""
    out, seen = [], {}
    for j in range(cfg.n_agents):
        p = int(cfg.agent_policy[j])
        out.append((p, seen.get(p, 0)))
        seen[p] = seen.get(p, 0) + 1
    return out


def record_rewards(ctx, cfg, records=None):
    """The fp32 rewards [T, N, n_agents] the context's records hold (records: per policy the
    arrays of records_get, read back when not given)."""
    T, N = cfg.frag_len, cfg.n_envs
    recs = records if records is not None else [ctx.records_get(p) for p in range(cfg.n_policies)]
    out = np.zeros((T, N, cfg.n_agents), np.float32)
    for j, (p, slot) in enumerate(agent_slots(cfg)):
        lay = ctx.layout[p]
        k = lay["C"] // N
        out[:, :, j] = recs[p].reshape(T, N, k, lay["stride"])[:, :, slot, lay["rew"]]
    return out
