"""PPOTrainer.evaluate_members and ddrl_amd.evaluation.evaluate_sweep on the device: the
published Local policies (tests/golden/ckpt_local_1250.npz, written out as an RLlib checkpoint
file) evaluated as members against PPOTrainer.evaluate of a trainer restored from the same file.

Reference: evaluation/evaluate_trained_policies_pd.py:84-127,
evaluation/evaluate_trained_policies_tvel_range_pd.py:59-118."""
import csv
import json
import os

import numpy as np
import pytest

from ddrl_amd import evaluation

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_local_1250.npz")
CFG = {"env": "QuantrupedMultiEnv_Local", "rollout_fragment_length": 8, "observation_filter": "MeanStdFilter"}
ARGS = dict(num_episodes=8, num_steps=30, explore=False)


def _fixture_states():
    z = np.load(FIX, allow_pickle=False)
    pids = json.loads(bytes(z["policy_ids"]).decode())
    return {pid: {"weights": z[f"{pid}/weights"], "adam_m": z[f"{pid}/adam_m"], "adam_v": z[f"{pid}/adam_v"],
                  "beta_powers": tuple(float(x) for x in z[f"{pid}/beta_powers"]),
                  "filter": (float(z[f"{pid}/filter_n"][0]), z[f"{pid}/filter_M"], z[f"{pid}/filter_S"]),
                  "kl_coeff": float(z[f"{pid}/kl_coeff"][0])} for pid in pids}


@pytest.fixture(scope="module")
def published(tmp_path_factory):
    """(path of the RLlib checkpoint file, evaluate() of a trainer restored from it)."""
    from ddrl_amd.trainer import PPOTrainer
    tr = PPOTrainer(CFG, n_envs=16, seed=2)
    tr.load_policy_states(_fixture_states())
    path = tr.save_rllib(str(tmp_path_factory.mktemp("ckpt")))
    tr.stop()
    ref = PPOTrainer(CFG, n_envs=16, seed=2)
    ref.restore_rllib(path)
    want = ref.evaluate(env_backend="device", n_envs=8, **ARGS)
    ref.stop()
    assert len(want[0]) == 8
    return path, want


def _trainer_state(tr):
    st = {"weights": tr.get_weights(), "filter": tr.ctx.filter_get(), "rfilter": tr.rctx.filter_get(),
          "adam": [tr.ctx.adam_get(p) for p in range(tr.cfg.n_policies)],
          "pf": [tr.ctx.policy_filter_get(p) for p in range(tr.cfg.n_policies)],
          "rweights": [tr.rctx.params_get(p) for p in range(tr.cfg.n_policies)]}
    return st


def _flat(x):
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in _flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [a for v in x for a in _flat(v)]
    return [np.asarray(x)]


def test_one_member_equals_evaluate(published):
    """A fresh trainer (its own weights are not the checkpoint's) evaluating the file as its only
    member returns the lists of evaluate() on a trainer restored from the file."""
    from ddrl_amd.trainer import PPOTrainer
    path, want = published
    tr = PPOTrainer(CFG, n_envs=16, seed=2)
    got = tr.evaluate_members([(path, None)], **ARGS)
    assert len(got) == 1
    for a, b in zip(got[0], want):
        assert a == b
    own = tr.evaluate(env_backend="device", n_envs=8, **ARGS)
    assert own[0] != want[0]          # the trainer's own weights give other episodes
    assert tr.evaluate_members([(None, None)], **ARGS)[0] == own
    tr.stop()


def test_member_zero_is_independent_and_the_trainer_is_untouched(published):
    from ddrl_amd.trainer import PPOTrainer
    path, want = published
    tr = PPOTrainer(CFG, n_envs=16, seed=2)
    before = _trainer_state(tr)
    got = tr.evaluate_members([(path, None), (None, None)], **ARGS)
    assert len(got) == 2
    for a, b in zip(got[0], want):   # member 0 owns envs 0..n-1; the env plane is keyed by env index
        assert a == b
    assert len(got[1][0]) == 8 and got[1][0] != got[0][0]
    for a, b in zip(_flat(before), _flat(_trainer_state(tr))):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match="at most 4096"):
        tr.evaluate_members([(None, None)] * 4097)
    with pytest.raises(ValueError, match="env_filter"):
        tr.evaluate_members([(None, None)], env_filter="other")
    with pytest.raises(ValueError, match="finite and > 0"):
        tr.evaluate_members([(None, -1.0)])
    tr.stop()


def test_evaluate_sweep(published, tmp_path):
    """The fixture's policies take 35 inputs, the TVel variant of the env feeds 36: the sweep runs
    on Local.  Without target velocities the rows are evaluate_checkpoints'; with them (labels of
    the per-env velocity table; the 43-column env does not observe the velocity) every row also
    carries target_velocity."""
    path, _ = published
    # the env-side filter is the sweep trainer's own (an RLlib checkpoint does not carry it), so the
    # rows to meet are evaluate_checkpoints', whose trainer is built the same way
    want = evaluation.evaluate_checkpoints(CFG, [path], "Local", seeds=[4], hf_smoothness=1.0, num_episodes=8,
                                           num_steps=30, n_envs=8, explore_during_rollout=False, env_backend="device")
    assert len(want) == 8
    rows = evaluation.evaluate_sweep(CFG, [path, path], "Local", seeds=[4, 7], hf_smoothness=1.0, **ARGS)
    assert len(rows) == 2 * 8 and all(list(r) == evaluation.COLUMNS for r in rows)
    assert [r["seed"] for r in rows] == [4] * 8 + [7] * 8
    assert [r["simulation_run"] for r in rows] == list(range(8)) * 2
    assert {r["approach"] for r in rows} == {"Local"} and {r["evaluated_on"] for r in rows} == {1.0}
    assert rows[:8] == want          # member 0 owns envs 0..7: evaluate_checkpoints' rows, column for column
    out = evaluation.write_csv(rows, str(tmp_path / "evaluation_1.0.csv"))
    with open(out, newline="") as f:
        back = list(csv.DictReader(f))
    assert list(back[0]) == evaluation.COLUMNS and len(back) == 16
    assert [float(r["reward"]) for r in back] == [r["reward"] for r in rows]

    rows = evaluation.evaluate_sweep(CFG, [path, path], "Local", target_velocities=[1.0, 2.0], **ARGS)
    assert len(rows) == 4 * 8 and all(set(r) == set(evaluation.COLUMNS_TVEL) for r in rows)
    assert [r["seed"] for r in rows] == [0] * 16 + [1] * 16                     # checkpoint-major
    assert [r["target_velocity"] for r in rows] == ([1.0] * 8 + [2.0] * 8) * 2
    assert [r["simulation_run"] for r in rows] == list(range(8)) * 4
    assert [r["reward"] for r in rows[:8]] == [r["reward"] for r in want]
    out = evaluation.write_csv(rows, str(tmp_path / "evaluation_tvel_range_1.0.csv"))
    with open(out, newline="") as f:
        back = list(csv.DictReader(f))
    assert list(back[0]) == evaluation.COLUMNS_TVEL and len(back) == 32
    assert [float(r["target_velocity"]) for r in back] == [r["target_velocity"] for r in rows]
    assert [float(r["CoT"]) for r in back] == [r["CoT"] for r in rows]
