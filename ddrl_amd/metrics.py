"""Episode metrics of a training run, as RLlib 1.0 reports them (pure numpy; nothing here
touches the device).

The rows come from `Context.episodes_collect()`: float64 [n, 8] =
{t, env, length, total, agent_0 .. agent_3} in ascending (t, env) order, one row per episode
that finished in the fragment (agents the env does not have are NaN).

RLlib 1.0 (3p evaluation/metrics.py summarize_episodes, 3p execution/metric_ops.py
CollectMetrics with metrics_smoothing_episodes = 100):
  * the new episodes are those that finished during the iteration; with fewer than `smoothing`
    of them the most recent (smoothing - n) older ones are put in front; the history is then
    extended with the new ones and cut to its last `smoothing`;
  * over that window: episode_reward_{max,min,mean} and episode_len_mean (nan when empty),
    policy_reward_{min,max,mean}[pid] over one entry per (agent, policy) pair per episode,
    hist_stats with the window's lists.
The result keys are the columns the reference's plotting scripts read from Tune's progress.csv
(visualization/visualize_learning_over_time.py:49-53: column 2 against column 6).
"""
from __future__ import annotations

import csv
import json
import numbers
import os

import numpy as np

EPISODE_KEYS = ("episode_reward_max", "episode_reward_min", "episode_reward_mean", "episode_len_mean",
                "episodes_this_iter", "policy_reward_min", "policy_reward_max", "policy_reward_mean",
                "custom_metrics", "hist_stats", "sampler_perf", "off_policy_estimator")


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
        # Array operations over the columns: the cost in Python does not grow with the row count (a
        # fragment of 4096 envs finishes thousands of episodes).  Only the kept history -- at most
        # `smoothing` episodes -- is ever held row by row.  The window's values and their order are
        # the per-row walk's, so np.min / np.max / np.mean see the same numbers in the same order.
        rows = np.asarray(rows, np.float64).reshape(-1, 8)
        agent_policy = [int(p) for p in agent_policy]
        n = rows.shape[0]
        missing = max(0, self.smoothing - n)
        old = self.history[-missing:] if missing > 0 else []
        keep = self._episodes(rows[n - min(n, self.smoothing):], agent_policy) if self.smoothing > 0 else []
        self.history = (self.history + keep)[-self.smoothing:] if self.smoothing > 0 else []

        def window(old_values, new_values, dtype):
            """(array, list) of the kept episodes' values followed by the new ones."""
            new_values = np.ascontiguousarray(new_values, dtype)
            if not old_values:
                return new_values, new_values.tolist()
            return np.concatenate([np.array(old_values, dtype), new_values]), old_values + new_values.tolist()

        r_arr, rewards = window([ep[0] for ep in old], rows[:, 3], np.float64)
        l_arr, lengths = window([ep[1] for ep in old], rows[:, 2].astype(np.int64), np.int64)
        nan = float("nan")
        hist = {"episode_reward": rewards, "episode_lengths": lengths}
        pmin, pmax, pmean = {}, {}, {}
        if rewards:
            # one entry per (agent, policy) pair per episode; the policies in the order of their first agent
            for p in dict.fromkeys(agent_policy):
                cols = [4 + j for j, q in enumerate(agent_policy) if q == p]
                a, rs = window([r for ep in old for q, r in ep[2] if q == p], rows[:, cols].ravel(), np.float64)
                pid = policy_ids[p]
                pmin[pid] = float(np.min(a))
                pmax[pid] = float(np.max(a))
                pmean[pid] = float(np.mean(a))
                hist[f"policy_{pid}_reward"] = rs
        return {
            "episode_reward_max": float(np.max(r_arr)) if rewards else nan,
            "episode_reward_min": float(np.min(r_arr)) if rewards else nan,
            "episode_reward_mean": float(np.mean(r_arr)) if rewards else nan,
            "episode_len_mean": float(np.mean(l_arr)) if lengths else nan,
            "episodes_this_iter": n,
            "policy_reward_min": pmin,
            "policy_reward_max": pmax,
            "policy_reward_mean": pmean,
            "custom_metrics": {},
            "hist_stats": hist,
            "sampler_perf": {},
            "off_policy_estimator": {},
        }


def merge_rank_rows(list_of_rows, n_envs_per_rank):
    """Every rank's rows -> one table with the global env index rank * N + env, sorted by
    (t, global env): the order a single process over the union of the envs would produce."""
    parts = []
    for rank, rows in enumerate(list_of_rows):
        r = np.array(rows, np.float64).reshape(-1, 8)
        r[:, 1] += rank * int(n_envs_per_rank)
        parts.append(r)
    allr = np.concatenate(parts) if parts else np.zeros((0, 8))
    order = np.lexsort((allr[:, 1], allr[:, 0]))
    return allr[order]


def gather_rank_rows(comm, rows, n_envs_per_rank):
    """This rank's rows -> the merged rows of every rank (the same array on every rank):
    counts and zero-padded rows go through comm.all_gather_np (ddrl_amd.ddp.Comm)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 8)
    counts = [int(c[0]) for c in comm.all_gather_np(np.array([rows.shape[0]], np.int64))]
    padded = np.zeros((max(max(counts), 1), 8), np.float64)
    padded[:rows.shape[0]] = rows
    parts = comm.all_gather_np(padded)
    return merge_rank_rows([part[:n] for part, n in zip(parts, counts)], n_envs_per_rank)


def flatten_result(result, skip=("hist_stats",)):
    """Tune's flatten_dict as its CSV logger applies it: scalar keys first in result order, then
    the nested keys flattened with "/" and appended (an empty dict leaves no column)."""
    flat = {k: v for k, v in result.items() if k not in skip}
    while any(isinstance(v, dict) for v in flat.values()):
        remove, add = [], {}
        for k, v in flat.items():
            if isinstance(v, dict):
                for sk, sv in v.items():
                    add[f"{k}/{sk}"] = sv
                remove.append(k)
        flat.update(add)
        for k in remove:
            del flat[k]
    return flat


def _jsonable(v):
    if isinstance(v, dict):
        return {str(k): _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, np.ndarray):
        return _jsonable(v.tolist())
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, numbers.Integral):
        return int(v)
    if isinstance(v, numbers.Real):
        return float(v)
    return v


class ProgressLogger:
    """Tune's CSV and JSON loggers for one trial: <logdir>/progress.csv (header from the first
    result, later lines keep its columns) and <logdir>/result.json (one JSON line per
    iteration, hist_stats included)."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        self.logdir = logdir
        self._csv = open(os.path.join(logdir, "progress.csv"), "w", newline="")
        self._json = open(os.path.join(logdir, "result.json"), "w")
        self._writer = None

    def on_result(self, result):
        result = _jsonable(result)
        json.dump(result, self._json)
        self._json.write("\n")
        self._json.flush()
        flat = {k: v for k, v in flatten_result(result).items() if not isinstance(v, (list, tuple))}
        if self._writer is None:
            self._writer = csv.DictWriter(self._csv, list(flat.keys()))
            self._writer.writeheader()
        self._writer.writerow({k: v for k, v in flat.items() if k in self._writer.fieldnames})
        self._csv.flush()

    def close(self):
        for f in (self._csv, self._json):
            if not f.closed:
                f.close()
