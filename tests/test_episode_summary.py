"""EpisodeHistory.summarize on array operations against the per-row implementation it replaced
(tests/episode_summary_reference.py, verbatim): every key, value, Python type and list order of
the result, and the kept history, over sequences of iterations that cross the smoothing window in
both directions.  It passes before and after the rewrite by construction: it guards the rewrite."""
import json

import numpy as np
import pytest

from ddrl_amd.metrics import EpisodeHistory, _jsonable
from tests.episode_summary_reference import EpisodeHistory as ReferenceHistory

MAPS = {"local": ([0, 1, 2, 3], ["p0", "p1", "p2", "p3"]),
        "shared": ([0, 0, 0, 0], ["shared"]),
        "sides": ([0, 0, 1, 1], ["left", "right"]),
        "single": ([0], ["central"])}
SEQUENCE = (0, 1, 99, 100, 101, 0, 5000, 1, 0)   # new rows per iteration


def _rows(rng, n, n_agents, t0):
    """n finished episodes as the device writes them: {t, env, length, total, agents (NaN past n_agents)}."""
    r = np.full((n, 8), np.nan)
    r[:, 0] = t0 + np.sort(rng.integers(0, 200, n))
    r[:, 1] = rng.integers(0, 4096, n)
    r[:, 2] = rng.integers(1, 1001, n)
    r[:, 4:4 + n_agents] = rng.normal(0.0, 50.0, (n, n_agents))
    r[:, 3] = r[:, 4:4 + n_agents].sum(1) * (1.0 + 1e-16)
    return r


def _same(a, b, path="result"):
    """Equality with the Python types of every entry (a float is not an int, a list not an array)."""
    assert type(a) is type(b), (path, type(a), type(b))
    if isinstance(a, dict):
        assert list(a.keys()) == list(b.keys()), path
        for k in a:
            _same(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif isinstance(a, float):
        assert (a == b) or (a != a and b != b), (path, a, b)
        assert np.float64(a).tobytes() == np.float64(b).tobytes() or (a != a and b != b), (path, a, b)
    else:
        assert a == b, (path, a, b)


@pytest.mark.parametrize("smoothing", [100, 5, 0])
@pytest.mark.parametrize("name", list(MAPS))
def test_summarize_equals_the_per_row_reference(name, smoothing):
    agent_policy, policy_ids = MAPS[name]
    rng = np.random.default_rng(1234 + smoothing)
    new, ref = EpisodeHistory(smoothing), ReferenceHistory(smoothing)
    for it, n in enumerate(SEQUENCE):
        rows = _rows(rng, n, len(agent_policy), 200 * it)
        before = rows.copy()
        got = new.summarize(rows, agent_policy, policy_ids)
        want = ref.summarize(rows, agent_policy, policy_ids)
        np.testing.assert_array_equal(rows, before)   # the caller's rows are left alone
        _same(got, want, f"iteration {it}")
        assert json.dumps(_jsonable(got)) == json.dumps(_jsonable(want))
        _same(new.history, ref.history, f"history after iteration {it}")
        assert len(new.history) <= max(smoothing, 0)


def test_empty_window_is_nan_with_empty_policy_dicts():
    out = EpisodeHistory(100).summarize(np.zeros((0, 8)), [0, 1, 2, 3], ["a", "b", "c", "d"])
    assert out["episodes_this_iter"] == 0 and type(out["episodes_this_iter"]) is int
    for k in ("episode_reward_max", "episode_reward_min", "episode_reward_mean", "episode_len_mean"):
        assert out[k] != out[k] and type(out[k]) is float
    assert out["policy_reward_mean"] == {} and out["hist_stats"] == {"episode_reward": [], "episode_lengths": []}


def test_rows_may_come_as_a_flat_or_integer_typed_sequence():
    rows = [[3, 1, 7, 2.5, 1.0, 1.5, float("nan"), float("nan")]]
    a = EpisodeHistory(10).summarize(rows, [0, 1], ["x", "y"])
    b = ReferenceHistory(10).summarize(rows, [0, 1], ["x", "y"])
    _same(a, b)
