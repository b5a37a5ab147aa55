"""Evaluation of trained policies with the reference's surface (evaluation/rollout_episodes.py:26-164,
evaluation/evaluate_trained_policies_pd.py:84-127): run a restored trainer for whole episodes and
report, per episode, reward, duration, distance, power, velocity and cost of transport.

The episodes run on the device path (PPOTrainer.evaluate: ddrl_eval_hostenv over the host env
plane, or ddrl_eval_devenv over the device env plane), n_envs envs side by side with a quota of
episodes each, not one after another.  `hf_smoothness` is the smoothness of the ground the
evaluation env plane is created with (the stand-in's procedural height field, csrc/envdyn.h): 1.0
is flat, and every episode of every env runs on ground of its own, as the reference regenerates
the field before every episode (evaluation/rollout_episodes.py:79).  The `evaluated_on` column of
evaluate_checkpoints' rows is the smoothness the episodes really ran on.
"""
from __future__ import annotations

import csv
import os

import numpy as np

COLUMNS = ["approach", "seed", "trained_on", "evaluated_on", "simulation_run", "reward", "duration", "distance",
           "power", "velocity", "CoT"]   # evaluate_trained_policies_pd.py:69


def rollout_episodes(env, agent, num_episodes=1, num_steps=1000, render=False, explore_during_rollout=None,
                     tvel=None, hf_smoothness=None, **evaluate_args):
    """rollout_episodes(env, agent, ...) of the reference: `agent` is a ddrl_amd PPOTrainer; `env` is
    accepted for the signature (the trainer evaluates on its own env plane; tvel sets the
    one-entry target-velocity list as the reference does on `env`, :38-39).  Returns
    (reward_eps, steps_eps, dist_eps, power_total_eps, vel_eps, cot_eps).
    explore_during_rollout None samples, as the reference's compute_action call without `explore`
    does (:103-107); False takes the action mean.  evaluate_args go to PPOTrainer.evaluate
    (n_envs, env_filter, seed, env_backend).  hf_smoothness: the ground's smoothness; None takes
    the trainer's env_config value (1.0 unless set)."""
    if render:
        raise NotImplementedError("rendering is out of scope: the host env plane has no viewer")
    explore = True if explore_during_rollout is None else bool(explore_during_rollout)
    return agent.evaluate(num_episodes=num_episodes, num_steps=num_steps, explore=explore, tvel=tvel,
                          hf_smoothness=hf_smoothness, **evaluate_args)


def default_sens_steps(n, S, rel_step=0.1, M=None):
    """The reference's perturbation steps (rollout_episodes_compute_gradient.py:62-66):
    rel_step * rs.std of a MeanStdFilter's RunningStat (n, M, S), std = sqrt(S / (n - 1)); while
    n <= 1 RLlib's RunningStat reports var = M^2 (0 when M is not given)."""
    S = np.asarray(S, np.float64)
    if n > 1:
        std = np.sqrt(S / (n - 1))
    else:
        std = np.abs(np.asarray(M, np.float64)) if M is not None else np.zeros_like(S)
    return float(rel_step) * std


def rollout_episodes_compute_gradient(env, agent, num_episodes=1, num_steps=1000, render=False, experiment_nr=0,
                                      tag="tvel1", out_dir=".", **evaluate_args):
    """rollout_episodes(env, agent, ...) of the reference's
    evaluation/rollout_episodes_compute_gradient.py:39-170 (driver:
    evaluation/generate_manual_gradients_targetvel.py): the evaluation episodes plus the importance
    matrix, written as grads_<tag>_<nr>.npy and grads_<tag>_abs_<nr>.npy ([d, A] float64, the files
    visualization/visualize_evaluated_grads_centralized.py reads) into out_dir.  The two files hold
    the first policy's matrices (the reference's central_policy); with several policies every
    policy also gets grads_<tag>_<nr>_<policy_id>.npy / grads_<tag>_abs_<nr>_<policy_id>.npy.
    `agent` is a ddrl_amd PPOTrainer; `env` is accepted for the signature.  evaluate_args go to
    PPOTrainer.evaluate_sensitivity (rel_step, steps, tvel, n_envs, env_filter, seed, explore).
    Returns (reward_eps, steps_eps, dist_eps, power_total_eps, vel_eps, cot_eps)."""
    if render:
        raise NotImplementedError("rendering is out of scope: the host env plane has no viewer")
    lists, sens = agent.evaluate_sensitivity(num_episodes=num_episodes, num_steps=num_steps, **evaluate_args)
    os.makedirs(out_dir, exist_ok=True)
    for k, (pid, res) in enumerate(sens.items()):
        for suffix in ([""] if k == 0 else []) + ([f"_{pid}"] if len(sens) > 1 else []):
            np.save(os.path.join(out_dir, f"grads_{tag}_{experiment_nr}{suffix}.npy"), res["grads"])
            np.save(os.path.join(out_dir, f"grads_{tag}_abs_{experiment_nr}{suffix}.npy"), res["grads_abs"])
    return lists


def evaluate_checkpoints(config, checkpoint_paths, approach, hf_smoothness=1.0, num_episodes=100, num_steps=1000,
                         seeds=None, trained_on="flat", n_envs=None, device=0, **evaluate_args):
    """evaluate_trained_policies_pd.py:84-127 for one approach: per checkpoint, build a trainer
    from `config`, restore the RLlib checkpoint, roll out num_episodes episodes and return one
    row (a dict with the reference's DataFrame columns, COLUMNS) per episode.  The episodes run
    on ground of smoothness hf_smoothness (the reference passes it as the env's hf_smoothness,
    :100-103); `evaluated_on` carries it."""
    from .trainer import PPOTrainer
    rows = []
    for k, path in enumerate(checkpoint_paths):
        agent = PPOTrainer(config, n_envs=8, device=device)   # the training shard is not used: a small one
        try:
            agent.restore_rllib(path)
            res = rollout_episodes(None, agent, num_episodes=num_episodes, num_steps=num_steps, n_envs=n_envs,
                                   hf_smoothness=hf_smoothness, **evaluate_args)
        finally:
            agent.stop()
        seed = seeds[k] if seeds is not None else k
        for it in range(len(res[0])):
            rows.append({"approach": approach, "seed": seed, "trained_on": trained_on, "evaluated_on": float(hf_smoothness),
                         "simulation_run": it, "reward": res[0][it], "duration": res[1][it], "distance": res[2][it],
                         "power": res[3][it], "velocity": res[4][it], "CoT": res[5][it]})
    return rows


# evaluate_trained_policies_tvel_range_pd.py:63: the same columns with target_velocity after evaluated_on
COLUMNS_TVEL = COLUMNS[:4] + ["target_velocity"] + COLUMNS[4:]
MAX_SWEEP_ENVS = 4096   # envs of one evaluate_members call


def evaluate_sweep(config, checkpoint_paths, approach, target_velocities=None, hf_smoothness=1.0, num_episodes=10,
                   num_steps=1000, seeds=None, trained_on="flat", device=0, **evaluate_args):
    """evaluate_checkpoints' rows for a whole sweep from ONE trainer and one evaluation per batch:
    the members are checkpoints x target velocities, checkpoint-major (the loops of
    evaluate_trained_policies_pd.py:84-127 and evaluate_trained_policies_tvel_range_pd.py:80-102),
    run side by side by PPOTrainer.evaluate_members on the device env plane.  The sweep is split
    into several evaluate_members calls when members x envs per member would pass 4096 envs.
    target_velocities None: one member per checkpoint at the configured velocity, COLUMNS rows;
    given: every row also carries `target_velocity` (COLUMNS_TVEL).  seeds: the `seed` label of
    each checkpoint (default: its index).  evaluate_args go to evaluate_members (explore,
    env_filter, seed)."""
    checkpoint_paths = list(checkpoint_paths)
    if not checkpoint_paths:
        raise ValueError("evaluate_sweep: no checkpoints")
    if seeds is not None and len(seeds) != len(checkpoint_paths):
        raise ValueError(f"evaluate_sweep: {len(seeds)} seed labels for {len(checkpoint_paths)} checkpoints")
    num_episodes = int(num_episodes)
    if num_episodes < 1:
        raise ValueError("evaluate_sweep: num_episodes must be >= 1")
    tvs = None
    if target_velocities is not None:
        tvs = [float(v) for v in np.asarray(target_velocities, np.float64).reshape(-1)]
        if not tvs or not all(np.isfinite(v) and v > 0.0 for v in tvs):
            raise ValueError("evaluate_sweep: target_velocities must be a non-empty list of finite values > 0")
    cells = [(k, path, tv) for k, path in enumerate(checkpoint_paths) for tv in (tvs or [None])]
    # members per call: every member keeps min(num_episodes, 4096 // M) envs, so M <= 4096 // envs wanted
    per_call = max(1, MAX_SWEEP_ENVS // min(num_episodes, MAX_SWEEP_ENVS))
    from .trainer import PPOTrainer
    agent = PPOTrainer(config, n_envs=8, device=device)   # the training shard is not used: a small one
    rows = []
    try:
        for i in range(0, len(cells), per_call):
            batch = cells[i:i + per_call]
            results = agent.evaluate_members([(path, tv) for _, path, tv in batch], num_episodes=num_episodes,
                                             num_steps=num_steps, hf_smoothness=hf_smoothness, **evaluate_args)
            for (k, _, tv), res in zip(batch, results):
                seed = seeds[k] if seeds is not None else k
                for it in range(len(res[0])):
                    row = {"approach": approach, "seed": seed, "trained_on": trained_on,
                           "evaluated_on": float(hf_smoothness), "simulation_run": it, "reward": res[0][it],
                           "duration": res[1][it], "distance": res[2][it], "power": res[3][it],
                           "velocity": res[4][it], "CoT": res[5][it]}
                    if tvs is not None:
                        row["target_velocity"] = tv
                    rows.append(row)
    finally:
        agent.stop()
    return rows


def write_csv(rows, path):
    """The rows as evaluation_<hf_smoothness>.csv (the csv module: pandas may be absent); with the
    target_velocity column (evaluation_tvel_range_<hf_smoothness>.csv) only when rows carry it."""
    rows = list(rows)
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=COLUMNS_TVEL if any("target_velocity" in r for r in rows) else COLUMNS)
        w.writeheader()
        w.writerows(rows)
    return path
