"""Evaluation of trained policies with the reference's surface (evaluation/rollout_episodes.py:26-164,
evaluation/evaluate_trained_policies_pd.py:84-127): run a restored trainer for whole episodes and
report, per episode, reward, duration, distance, power, velocity and cost of transport.

The episodes run on the device path (PPOTrainer.evaluate: ddrl_eval_hostenv over the host env
plane), n_envs envs side by side with a quota of episodes each, not one after another.  The
stand-in env has no terrain: `hf_smoothness` is carried into the rows as a label only.
"""
from __future__ import annotations

import csv

COLUMNS = ["approach", "seed", "trained_on", "evaluated_on", "simulation_run", "reward", "duration", "distance",
           "power", "velocity", "CoT"]   # evaluate_trained_policies_pd.py:69


def rollout_episodes(env, agent, num_episodes=1, num_steps=1000, render=False, explore_during_rollout=None,
                     tvel=None, **evaluate_args):
    """rollout_episodes(env, agent, ...) of the reference: `agent` is a ddrl_amd PPOTrainer; `env` is
    accepted for the signature (the trainer evaluates on its own env plane; tvel sets the
    one-entry target-velocity list as the reference does on `env`, :38-39).  Returns
    (reward_eps, steps_eps, dist_eps, power_total_eps, vel_eps, cot_eps).
    explore_during_rollout None samples, as the reference's compute_action call without `explore`
    does (:103-107); False takes the action mean.  evaluate_args go to PPOTrainer.evaluate
    (n_envs, env_filter, seed)."""
    if render:
        raise NotImplementedError("rendering is out of scope: the host env plane has no viewer")
    explore = True if explore_during_rollout is None else bool(explore_during_rollout)
    return agent.evaluate(num_episodes=num_episodes, num_steps=num_steps, explore=explore, tvel=tvel,
                          **evaluate_args)


def evaluate_checkpoints(config, checkpoint_paths, approach, hf_smoothness=1.0, num_episodes=100, num_steps=1000,
                         seeds=None, trained_on="flat", n_envs=None, device=0, **evaluate_args):
    """evaluate_trained_policies_pd.py:84-127 for one approach: per checkpoint, build a trainer
    from `config`, restore the RLlib checkpoint, roll out num_episodes episodes and return one
    row (a dict with the reference's DataFrame columns, COLUMNS) per episode."""
    from .trainer import PPOTrainer
    rows = []
    for k, path in enumerate(checkpoint_paths):
        cfg = {**config, "env_config": {**config.get("env_config", {}), "hf_smoothness": hf_smoothness}}
        agent = PPOTrainer(cfg, n_envs=8, device=device)   # the training shard is not used: a small one
        try:
            agent.restore_rllib(path)
            res = rollout_episodes(None, agent, num_episodes=num_episodes, num_steps=num_steps, n_envs=n_envs,
                                   **evaluate_args)
        finally:
            agent.stop()
        seed = seeds[k] if seeds is not None else k
        for it in range(len(res[0])):
            rows.append({"approach": approach, "seed": seed, "trained_on": trained_on, "evaluated_on": hf_smoothness,
                         "simulation_run": it, "reward": res[0][it], "duration": res[1][it], "distance": res[2][it],
                         "power": res[3][it], "velocity": res[4][it], "CoT": res[5][it]})
    return rows


def write_csv(rows, path):
    """The rows as evaluation_<hf_smoothness>.csv (the csv module: pandas may be absent)."""
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=COLUMNS)
        w.writeheader()
        w.writerows(rows)
    return path
