"""Host side of the episode metrics (ddrl_amd.metrics, pure numpy): RLlib 1.0's smoothing window
and summary against the results RLlib itself recorded at the end of the published runs
(tests/golden/episode_metrics.json, from Results/**/experiment_state-*.json), the cross-rank
merge against the single-process order, and Tune's progress.csv / result.json layout.

The recorded summary values are np.mean / np.min / np.max of the recorded hist_stats lists, so
replaying those lists through EpisodeHistory must give them bit for bit: no tolerance."""
import csv
import json
import math
import os
import socket
import tempfile

import numpy as np
import pytest

from ddrl_amd.metrics import EPISODE_KEYS, EpisodeHistory, ProgressLogger, flatten_result, merge_rank_rows
from ddrl_amd.spec import make_cfg
from tests.episodes_reference import EpisodeReference, agent_slots

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "episode_metrics.json")
with open(GOLDEN) as _fh:
    RECORDED = json.load(_fh)


def _recorded_rows(rec, cfg, policy_ids):
    """The window of a recorded result as collect rows: episode i's total and length, and agent
    j's total from its policy's list (k entries per episode, in agent order)."""
    h = rec["hist_stats"]
    n = len(h["episode_reward"])
    rows = np.full((n, 8), np.nan)
    k = [sum(1 for p, _ in agent_slots(cfg) if p == q) for q in range(cfg.n_policies)]
    for i in range(n):
        rows[i, :4] = [i, 0, h["episode_lengths"][i], h["episode_reward"][i]]
        for j, (p, slot) in enumerate(agent_slots(cfg)):
            rows[i, 4 + j] = h[f"policy_{policy_ids[p]}_reward"][i * k[p] + slot]
    return rows


def test_fixture_covers_the_architectures():
    assert {"Centralized", "TwoDiags", "TwoSides", "Centralized_TVel", "FullyDecentral_TVel", "Local_TVel",
            "TwoSides_TVel"} <= set(RECORDED)
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("arch", sorted(RECORDED))
def test_recorded_results_bit_for_bit(arch):
    rec = RECORDED[arch]
    cfg, inst = make_cfg("QuantrupedMultiEnv_" + arch.replace("_TVel", ""), 1, 1)
    policy_ids = list(type(inst).policy_names)
    assert set(policy_ids) == set(rec["policy_reward_mean"])
    rows = _recorded_rows(rec, cfg, policy_ids)
    n_new = rec["episodes_this_iter"]
    assert 0 < n_new < 100 and rows.shape[0] == 100
    hist = EpisodeHistory(100)
    agent_policy = [p for p, _ in agent_slots(cfg)]
    hist.summarize(rows[:100 - n_new], agent_policy, policy_ids)       # the older episodes
    out = hist.summarize(rows[100 - n_new:], agent_policy, policy_ids)
    assert list(out) == rec["key_order"][:len(out)] == list(EPISODE_KEYS)
    for k in ("episode_reward_max", "episode_reward_min", "episode_reward_mean", "episode_len_mean",
              "episodes_this_iter"):
        assert out[k] == rec[k] and type(out[k]) is type(rec[k]), (k, out[k], rec[k])
    for k in ("policy_reward_min", "policy_reward_max", "policy_reward_mean"):
        assert out[k] == rec[k], k                                    # dict of floats: exact
        assert list(out[k]) == list(rec[k])
    assert out["hist_stats"] == rec["hist_stats"]
    assert list(out["hist_stats"]) == list(rec["hist_stats"])
    assert out["custom_metrics"] == {} and out["sampler_perf"] == {} and out["off_policy_estimator"] == {}
    if cfg.n_policies > 1:   # the interleaved total is not the sum of the per-policy totals
        s = np.nansum(rows[:, 4:], axis=1)
        assert 0 < np.abs(s - rows[:, 3]).max() < 1e-9


def _rows(rng, n, n_agents=4, t0=0):
    r = np.full((n, 8), np.nan)
    r[:, 0] = t0 + np.sort(rng.integers(0, 50, size=n))
    r[:, 1] = np.arange(n)
    r[:, 2] = rng.integers(1, 1000, size=n)
    r[:, 4:4 + n_agents] = rng.normal(size=(n, n_agents)) * 100
    r[:, 3] = r[:, 4:4 + n_agents].sum(axis=1) + rng.normal(size=n) * 1e-11
    return r


def test_empty_window_gives_nan_and_no_policy_keys():
    out = EpisodeHistory(100).summarize(np.zeros((0, 8)), [0, 1, 2, 3], ["a", "b", "c", "d"])
    assert list(out) == list(EPISODE_KEYS)
    for k in ("episode_reward_max", "episode_reward_min", "episode_reward_mean", "episode_len_mean"):
        assert math.isnan(out[k])
    assert out["episodes_this_iter"] == 0
    assert out["policy_reward_min"] == out["policy_reward_max"] == out["policy_reward_mean"] == {}
    assert out["hist_stats"] == {"episode_reward": [], "episode_lengths": []}


@pytest.mark.parametrize("n_new", [99, 100, 101])
def test_window_after_a_full_history(n_new):
    rng = np.random.default_rng(n_new)
    ids, ap = ["a", "b", "c", "d"], [0, 1, 2, 3]
    h = EpisodeHistory(100)
    old = _rows(rng, 100)
    first = h.summarize(old, ap, ids)
    assert first["episodes_this_iter"] == 100 and first["hist_stats"]["episode_reward"] == old[:, 3].tolist()
    new = _rows(rng, n_new)
    out = h.summarize(new, ap, ids)
    # fewer than 100 new: the most recent 100 - n older ones in front; otherwise all the new ones
    window = np.concatenate([old[-(100 - n_new):], new]) if n_new < 100 else new
    assert out["episodes_this_iter"] == n_new
    assert out["hist_stats"]["episode_reward"] == window[:, 3].tolist()
    assert out["hist_stats"]["episode_lengths"] == window[:, 2].astype(int).tolist()
    assert out["episode_reward_mean"] == np.mean(window[:, 3].tolist())
    assert out["episode_reward_max"] == window[:, 3].max() and out["episode_reward_min"] == window[:, 3].min()
    assert out["episode_len_mean"] == np.mean(window[:, 2].astype(int).tolist())
    assert out["policy_reward_mean"]["c"] == np.mean(window[:, 6].tolist())
    # the history is cut to its last 100, older entries first
    assert len(h.history) == 100
    assert [ep[0] for ep in h.history] == np.concatenate([old, new])[-100:, 3].tolist()
    nxt = h.summarize(np.zeros((0, 8)), ap, ids)
    assert nxt["episodes_this_iter"] == 0
    assert nxt["hist_stats"]["episode_reward"] == np.concatenate([old, new])[-100:, 3].tolist()


def test_shared_policy_gives_four_entries_per_episode():
    rng = np.random.default_rng(1)
    rows = _rows(rng, 7)
    out = EpisodeHistory(100).summarize(rows, [0, 0, 0, 0], ["policy_legs"])
    assert out["hist_stats"]["policy_policy_legs_reward"] == rows[:, 4:8].reshape(-1).tolist()
    assert out["policy_reward_min"] == {"policy_legs": rows[:, 4:8].min()}
    assert out["policy_reward_mean"] == {"policy_legs": np.mean(rows[:, 4:8].reshape(-1).tolist())}
    # a one-agent env: one entry per episode, the NaN columns are not agents
    one = _rows(rng, 5, n_agents=1)
    out = EpisodeHistory(100).summarize(one, [0], ["central_policy"])
    assert out["hist_stats"]["policy_central_policy_reward"] == one[:, 4].tolist()


def test_smoothing_is_configurable():
    rng = np.random.default_rng(2)
    h = EpisodeHistory(3)
    a, b = _rows(rng, 5), _rows(rng, 1)
    h.summarize(a, [0], ["p"])
    out = h.summarize(b, [0], ["p"])
    assert out["hist_stats"]["episode_reward"] == a[-2:, 3].tolist() + b[:, 3].tolist()


# ---- merge across ranks ---------------------------------------------------------------------
def _rank_fragments(world, n_envs, T, seed):
    """Per-rank rewards / dones, the per-rank rows and the rows of one process over all envs."""
    rng = np.random.default_rng(seed)
    rew = rng.normal(size=(T, world * n_envs, 2)).astype(np.float32)
    done = (rng.random(size=(T, world * n_envs)) < 0.3).astype(np.uint8)
    done[3, :] = 1                                                     # ties in t on every rank
    single = EpisodeReference(world * n_envs, 2).fragment(rew, done)
    per_rank = [EpisodeReference(n_envs, 2).fragment(rew[:, r * n_envs:(r + 1) * n_envs],
                                                     done[:, r * n_envs:(r + 1) * n_envs]) for r in range(world)]
    return per_rank, single


@pytest.mark.parametrize("world", [2, 3])
def test_merge_rank_rows_is_the_single_process_order(world):
    per_rank, single = _rank_fragments(world, 5, 9, 40 + world)
    keep = [r.copy() for r in per_rank]
    np.testing.assert_array_equal(merge_rank_rows(per_rank, 5), single)
    for a, b in zip(per_rank, keep):                                   # the inputs are left as they were
        np.testing.assert_array_equal(a, b)
    empty = merge_rank_rows([np.zeros((0, 8)), per_rank[1]], 5)
    assert empty.shape == per_rank[1].shape and (empty[:, 1] >= 5).all()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gather_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from ddrl_amd.ddp import Comm
    from ddrl_amd.metrics import gather_rank_rows
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    per_rank, _ = _rank_fragments(world, 5, 9, 77)
    merged = gather_rank_rows(Comm("cpu"), per_rank[rank], 5)
    none = gather_rank_rows(Comm("cpu"), np.zeros((0, 8)), 5)         # no episode anywhere
    np.savez(os.path.join(out_dir, f"m{rank}.npz"), merged=merged, none=none)
    dist.destroy_process_group()


def test_gather_rank_rows_through_gloo():
    import torch.multiprocessing as mp
    out = tempfile.mkdtemp()
    mp.spawn(_gather_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    _, single = _rank_fragments(2, 5, 9, 77)
    for r in range(2):                                                 # every rank reports the same rows
        z = np.load(os.path.join(out, f"m{r}.npz"))
        np.testing.assert_array_equal(z["merged"], single)
        assert z["none"].shape == (0, 8)


# ---- progress.csv / result.json ---------------------------------------------------------------
COLUMNS_0_6 = ["episode_reward_max", "episode_reward_min", "episode_reward_mean", "episode_len_mean",
               "episodes_this_iter", "num_healthy_workers", "timesteps_total"]


def _result(rng, ids, agent_policy, hist, it, n):
    out = hist.summarize(_rows(rng, n, n_agents=len(agent_policy)), agent_policy, ids)
    out.update({"num_healthy_workers": 1, "timesteps_total": 1600 * it,
                "timers": {"sample_time_ms": 1.5, "learn_time_ms": 2.5},
                "info": {"learner": {pid: {"kl": 0.01 * it, "total_loss": np.float32(0.5)} for pid in ids}},
                "done": False, "episodes_total": 3 * it, "training_iteration": it})
    return out


@pytest.mark.parametrize("ids,agent_policy", [(["central_policy"], [0]),
                                              (["policy_FL", "policy_HL", "policy_HR", "policy_FR"], [0, 1, 2, 3])])
def test_progress_logger_columns_and_round_trip(tmp_path, ids, agent_policy):
    rng = np.random.default_rng(3)
    hist = EpisodeHistory(100)
    results = [_result(rng, ids, agent_policy, hist, it, n) for it, n in ((1, 3), (2, 0), (3, 4))]
    log = ProgressLogger(str(tmp_path / "trial"))
    for r in results:
        log.on_result(r)
    log.close()
    with open(tmp_path / "trial" / "progress.csv", newline="") as fh:
        lines = list(csv.reader(fh))
    header = lines[0]
    assert header[:7] == COLUMNS_0_6
    assert len(lines) == 4 and all(len(ln) == len(header) for ln in lines)   # header-stable later lines
    assert not any(c.startswith("hist_stats") for c in header)
    assert f"policy_reward_mean/{ids[-1]}" in header and f"info/learner/{ids[0]}/kl" in header
    assert header.index("done") < header.index("policy_reward_min/" + ids[0])   # nested keys appended
    for ln, r in zip(lines[1:], results):
        assert float(ln[2]) == r["episode_reward_mean"] and int(ln[6]) == r["timesteps_total"]
        assert int(ln[4]) == r["episodes_this_iter"]
    assert list(flatten_result(results[0]))[:7] == COLUMNS_0_6
    with open(tmp_path / "trial" / "result.json") as fh:
        back = [json.loads(ln) for ln in fh]
    assert len(back) == 3
    for b, r in zip(back, results):
        assert list(b) == list(r)
        assert b["hist_stats"] == r["hist_stats"] and b["episode_reward_mean"] == r["episode_reward_mean"]
        assert b["policy_reward_mean"] == r["policy_reward_mean"]
        assert b["info"]["learner"][ids[0]]["total_loss"] == 0.5


def test_progress_logger_writes_nan_for_an_empty_window(tmp_path):
    hist = EpisodeHistory(100)
    r = _result(np.random.default_rng(0), ["p"], [0], hist, 1, 0)
    log = ProgressLogger(str(tmp_path))
    log.on_result(r)
    log.close()
    with open(tmp_path / "progress.csv", newline="") as fh:
        lines = list(csv.reader(fh))
    assert lines[0][:7] == COLUMNS_0_6 and math.isnan(float(lines[1][2]))
    with open(tmp_path / "result.json") as fh:
        assert math.isnan(json.loads(fh.readline())["episode_reward_mean"])
