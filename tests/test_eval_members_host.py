"""Host side of the evaluation members: argument validation of PPOTrainer.evaluate_members, the
splitting and labelling of ddrl_amd.evaluation.evaluate_sweep (the trainer stubbed: no device), and
write_csv's column rule (evaluation/evaluate_trained_policies_pd.py:69 against
evaluation/evaluate_trained_policies_tvel_range_pd.py:63)."""
import csv

import pytest

from ddrl_amd import evaluation, native as N


def _bare_trainer():
    from ddrl_amd.trainer import PPOTrainer
    return object.__new__(PPOTrainer)   # the checks below run before anything of the trainer is read


def test_evaluate_members_validates_before_touching_the_device():
    tr = _bare_trainer()
    with pytest.raises(ValueError, match="4097 members, at most 4096"):
        tr.evaluate_members([(None, None)] * 4097)
    with pytest.raises(ValueError, match="at least one member"):
        tr.evaluate_members([])
    with pytest.raises(ValueError, match="pairs"):
        tr.evaluate_members([(None, 1.0, 2.0)])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and > 0"):
            tr.evaluate_members([(None, 1.0), (None, bad)])
    with pytest.raises(ValueError, match="env_filter"):
        tr.evaluate_members([(None, None)], env_filter="other")
    with pytest.raises(ValueError, match="num_episodes and num_steps"):
        tr.evaluate_members([(None, None)], num_episodes=0)


class _StubTrainer:
    """Stands in for PPOTrainer: records every evaluate_members call, returns labelled lists."""
    made = []

    def __init__(self, config, n_envs=None, device=0):
        self.config, self.calls, self.stopped = config, [], False
        _StubTrainer.made.append(self)

    def evaluate_members(self, members, num_episodes=10, num_steps=1000, **kw):
        self.calls.append((list(members), num_episodes, num_steps, kw))
        out = []
        for path, tv in members:
            tag = float(path.split("_")[-1]) * 100 + (tv or 0.0)
            col = [tag + it for it in range(num_episodes)]
            out.append((col, [num_steps] * num_episodes, col, col, col, col))
        return out

    def stop(self):
        self.stopped = True


@pytest.fixture
def stub(monkeypatch):
    import ddrl_amd.trainer as T
    _StubTrainer.made = []
    monkeypatch.setattr(T, "PPOTrainer", _StubTrainer)
    return _StubTrainer


def test_evaluate_sweep_labels_rows(stub):
    paths = ["ck_1", "ck_2", "ck_3"]
    rows = evaluation.evaluate_sweep({"env": "x"}, paths, "Local", target_velocities=[0.5, 1.5], hf_smoothness=0.8,
                                     num_episodes=3, num_steps=40, seeds=[5, 6, 7], trained_on="curriculum",
                                     explore=False)
    assert len(stub.made) == 1 and stub.made[0].stopped               # one trainer for the whole sweep
    (members, ne, ns, kw), = stub.made[0].calls
    assert members == [(p, tv) for p in paths for tv in (0.5, 1.5)]    # checkpoint-major
    assert (ne, ns) == (3, 40) and kw == {"hf_smoothness": 0.8, "explore": False}
    assert len(rows) == 6 * 3
    assert [r["seed"] for r in rows] == [s for s in (5, 6, 7) for _ in range(6)]
    assert [r["target_velocity"] for r in rows] == [tv for _ in paths for tv in (0.5, 1.5) for _ in range(3)]
    assert [r["simulation_run"] for r in rows] == [0, 1, 2] * 6
    assert {r["trained_on"] for r in rows} == {"curriculum"} and {r["evaluated_on"] for r in rows} == {0.8}
    assert rows[4]["reward"] == 100 + 1.5 + 1 and rows[4]["duration"] == 40    # ck_1, tv 1.5, run 1
    assert all(set(r) == set(evaluation.COLUMNS_TVEL) for r in rows)

    rows = evaluation.evaluate_sweep({"env": "x"}, paths, "Local", num_episodes=2)
    assert stub.made[1].calls[0][0] == [(p, None) for p in paths]
    assert [r["seed"] for r in rows] == [0, 0, 1, 1, 2, 2]
    assert all(list(r) == evaluation.COLUMNS for r in rows)


def test_evaluate_sweep_splits_past_4096_envs(stub):
    paths = [f"ck_{i}" for i in range(5)]
    rows = evaluation.evaluate_sweep({"env": "x"}, paths, "Local", target_velocities=[1.0, 2.0], num_episodes=1500)
    calls = stub.made[0].calls
    assert [len(c[0]) for c in calls] == [2] * 5                        # 4096 // 1500 members per call
    assert [m for c in calls for m in c[0]] == [(p, tv) for p in paths for tv in (1.0, 2.0)]
    assert len(rows) == 10 * 1500
    assert [r["seed"] for r in rows[::1500]] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    # more episodes than one evaluation has envs: one member per call
    evaluation.evaluate_sweep({"env": "x"}, paths[:2], "Local", num_episodes=5000, num_steps=1)
    assert [len(c[0]) for c in stub.made[1].calls] == [1, 1]


def test_evaluate_sweep_validates(stub):
    with pytest.raises(ValueError, match="no checkpoints"):
        evaluation.evaluate_sweep({}, [], "Local")
    with pytest.raises(ValueError, match="seed labels"):
        evaluation.evaluate_sweep({}, ["ck_1", "ck_2"], "Local", seeds=[1])
    with pytest.raises(ValueError, match="num_episodes"):
        evaluation.evaluate_sweep({}, ["ck_1"], "Local", num_episodes=0)
    for bad in ([], [1.0, 0.0], [float("nan")], [-2.0]):
        with pytest.raises(ValueError, match="target_velocities"):
            evaluation.evaluate_sweep({}, ["ck_1"], "Local", target_velocities=bad)
    assert stub.made == []                                              # refused before a trainer is built


def test_write_csv_gains_the_column_only_when_rows_carry_it(tmp_path):
    base = {"approach": "Local", "seed": 1, "trained_on": "flat", "evaluated_on": 1.0, "simulation_run": 0,
            "reward": 1.5, "duration": 7, "distance": 0.25, "power": 2.0, "velocity": 0.125, "CoT": 3.0}

    def header_and_rows(rows, name):
        with open(evaluation.write_csv(rows, str(tmp_path / name)), newline="") as f:
            r = csv.reader(f)
            return next(r), list(r)

    head, body = header_and_rows([base], "a.csv")
    assert head == evaluation.COLUMNS == ["approach", "seed", "trained_on", "evaluated_on", "simulation_run", "reward",
                                          "duration", "distance", "power", "velocity", "CoT"]
    assert body == [["Local", "1", "flat", "1.0", "0", "1.5", "7", "0.25", "2.0", "0.125", "3.0"]]
    head, body = header_and_rows([{**base, "target_velocity": 1.5}], "b.csv")
    assert head == ["approach", "seed", "trained_on", "evaluated_on", "target_velocity", "simulation_run", "reward",
                    "duration", "distance", "power", "velocity", "CoT"]            # tvel_range_pd.py:63
    assert body[0][4] == "1.5" and body[0][5] == "0"
    head, _ = header_and_rows([], "c.csv")
    assert head == evaluation.COLUMNS


def test_bindings_declare_the_member_calls():
    for name in ("ddrl_eval_members_begin", "ddrl_eval_member_load", "ddrl_eval_member_filter_get",
                 "ddrl_devenv_set_env_target_velocities"):
        assert name in N._SIGS and name in N.header_symbols()
