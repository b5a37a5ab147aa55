"""fp64 numpy restatement of the evaluation path, for the evaluation tests.

Written from the arithmetic of the reference's evaluation/rollout_episodes.py:
  :122      reward_total += sum(reward.values())          (Python floats, agent order)
  :146-147  power_total += np.sum(np.abs(np.roll(ctrl, -2) * qvel[6:]))
  :149-151  distance = qpos[0] - start; velocity = distance / steps;
            CoT = (power_total / steps) / (total_mass * velocity)
applied to N envs with a quota of E episodes each (rows past the quota are ignored, rows not
reached stay NaN), and a deterministic-action variant of the harness's OracleRollout
(filters with `update` per flag, per-policy filters never updated, clip(mean) when no noise).
"""
import numpy as np

from oracle import ddrl_oracle as O

TOTAL_MASS = 8.78710174560547   # rollout_episodes.py:152


def step_rewards(cfg, inst, fw, cfrc, actions):
    """Per env: sum(reward.values()) of one step, as a Python float (fp64), agents in order."""
    agents = list(inst.agent_names)
    tables = {a: (inst.contact_force_indices[a][0], inst.contact_force_indices[a][1]) for a in agents}
    out = []
    for e in range(fw.shape[0]):
        ad = {a: actions[e, inst.action_indices[a]].astype(np.float64) for a in agents}
        if inst.reward_mode == "global":
            rw = O.global_reward(float(fw[e]), cfrc[e].astype(np.float64), ad, cfg.ctrl_cost_weight,
                                 cfg.contact_cost_weight)
        else:
            rw = O.per_leg_reward(float(fw[e]), cfrc[e].astype(np.float64), ad, tables, cfg.ctrl_cost_weight,
                                  cfg.contact_cost_weight, norm_reward=inst.reward_mode == "norm")
        out.append(sum(float(rw[a]) for a in agents))
    return out


class EpisodeAccumulator:
    """The per-env accumulators and the result table [N][E][6] =
    {return, steps, distance, power, velocity, CoT}."""

    def __init__(self, n_envs, episodes_per_env, total_mass=TOTAL_MASS, ctrl_roll=2):
        self.N, self.E, self.mass, self.roll = n_envs, episodes_per_env, total_mass, ctrl_roll
        self.ret = [0.0] * n_envs
        self.power = [0.0] * n_envs
        self.dist = [0.0] * n_envs
        self.steps = [0] * n_envs
        self.count = [0] * n_envs
        self.table = np.full((n_envs, episodes_per_env, 6), np.nan)

    def step(self, rewards, actions, kin, done):
        """rewards: per env the step's summed reward (step_rewards); actions [N, 8] the clipped env
        actions (= sim.data.ctrl); kin [N, 9] = {dx, joint qvel[8]}; done [N]."""
        for e in range(self.N):
            ctrl = np.asarray(actions[e], np.float64)
            qvel = np.asarray(kin[e, 1:9], np.float64)
            self.ret[e] += float(rewards[e])
            self.power[e] += float(np.sum(np.abs(np.roll(ctrl, -self.roll) * qvel)))
            self.dist[e] += float(kin[e, 0])
            self.steps[e] += 1
            if not done[e]:
                continue
            if self.count[e] < self.E:
                with np.errstate(divide="ignore", invalid="ignore"):   # IEEE results at distance 0
                    vel = np.float64(self.dist[e]) / np.float64(self.steps[e])
                    cot = (np.float64(self.power[e]) / np.float64(self.steps[e])) / (np.float64(self.mass) * vel)
                self.table[e, self.count[e]] = [self.ret[e], self.steps[e], self.dist[e], self.power[e], vel, cot]
                self.count[e] += 1
            self.ret[e] = self.power[e] = self.dist[e] = 0.0
            self.steps[e] = 0

    @property
    def episodes_done(self):
        return int(sum(self.count))

    @property
    def envs_finished(self):
        return int(sum(c == self.E for c in self.count))


def scripted_done(T, n, seed=41, p=0.25):
    """The seeded done pattern [T, n] of the scripted accounting tests."""
    return (np.random.default_rng(seed).random((T, n)) < p).astype(np.uint8)


def done_classes(done, E):
    """How many envs of a done pattern fall into each class the accounting has to handle with a
    quota of E episodes: never filling it (some without any episode), exactly E ends, more,
    stepped after the quota is full, and the number of one-step episodes."""
    done = np.asarray(done, bool)
    T, n = done.shape
    cnt = done.sum(0)
    last_quota = np.array([np.flatnonzero(done[:, e])[E - 1] if cnt[e] >= E else T * 10 for e in range(n)])
    one_step = sum(int(done[0, e]) + int((done[1:, e] & done[:-1, e]).sum()) for e in range(n))
    return dict(never_fill=int((cnt < E).sum()), no_episode=int((cnt == 0).sum()), exactly=int((cnt == E).sum()),
                more=int((cnt > E).sum()), stepped_after_quota=int((last_quota < T - 1).sum()), one_step=one_step)


def eval_observe(orc, obs, filter_update):
    """OracleRollout._observe_block for evaluation: the env-side filter pushes only with
    filter_update, the per-policy filters normalize without update (compute_action)."""
    cfg = orc.cfg
    normed = O.mean_std_filter(obs, orc.rs, update=bool(filter_update), clip=cfg.filter_clip)
    tables = orc.model_tables()
    ext = np.concatenate([normed, np.zeros((normed.shape[0], 1)), np.ones((normed.shape[0], 1))], 1)
    col = lambda i: i if i >= 0 else normed.shape[1] + (-1 - i)
    stage = []
    for p in range(cfg.n_policies):
        cols = [ext[:, [col(i) for i in tables[a]]] for a in orc.slots[p]]
        x = np.stack(cols, 1).reshape(-1, cfg.obs_dim[p])
        if orc.pf is not None:
            x = O.mean_std_filter(x, orc.pf[p], update=False, clip=None)
        stage.append(x.astype(np.float32))
    orc.stage = stage
    return stage


def eval_act(orc, eps=None):
    """(env actions [N, 8], logits per policy) of the staged observation: the mean (eps None,
    explore=False) or mean + std * eps, clipped and scattered like OracleRollout.act."""
    cfg = orc.cfg
    A = cfg.act_dim
    actions = np.zeros((cfg.n_envs, 8), np.float32)
    all_logits = []
    for p in range(cfg.n_policies):
        logits, _, _ = orc.forward(p, orc.stage[p])
        all_logits.append(logits)
        k = len(orc.slots[p])
        if eps is None:
            a = logits[:, :A]
        else:
            e_idx = [orc.agents.index(n) for n in orc.slots[p]]
            a = O.dg_sample(logits, eps[:, e_idx, :].reshape(-1, A))
        for s, name in enumerate(orc.slots[p]):
            sign = np.where(getattr(orc.inst, "action_negate", {}).get(name, [False] * A), -1.0, 1.0)
            actions[:, orc.inst.action_indices[name]] = np.clip(a.reshape(-1, k, A)[:, s], -1, 1) * sign
    return actions, all_logits
