"""PPOTrainer.evaluate_sensitivity and ddrl_amd.evaluation.rollout_episodes_compute_gradient over the
device path: the reference's importance-matrix surface
(evaluation/rollout_episodes_compute_gradient.py:39-170, driven by
evaluation/generate_manual_gradients_targetvel.py; the files
visualization/visualize_evaluated_grads_centralized.py reads)."""
import os

import numpy as np
import pytest

from ddrl_amd import evaluation

pytestmark = pytest.mark.gpu
CFG = {"env": "QuantrupedMultiEnv_Local", "rollout_fragment_length": 8}
ARGS = dict(num_episodes=4, num_steps=20, n_envs=2, seed=3)


def _check(tr, lists, sens):
    d, A = int(tr.cfg.obs_dim[0]), tr.cfg.act_dim
    assert list(sens) == list(tr.policy_ids)
    for pid, res in sens.items():
        assert set(res) == {"grads", "grads_abs", "rows"}
        assert res["grads"].shape == res["grads_abs"].shape == (d, A) and res["grads"].dtype == np.float64
        assert res["rows"] == sum(lists[1])   # one row per policy and env step of the reported episodes
        assert np.isfinite(res["grads"]).all() and (np.abs(res["grads"]) <= res["grads_abs"]).all()
        assert (res["grads_abs"] > 0).mean() >= 0.9


def test_evaluate_sensitivity_returns_evaluates_lists_and_the_matrices():
    from ddrl_amd.trainer import PPOTrainer
    tr = PPOTrainer(CFG, n_envs=16, seed=3)
    want = tr.evaluate(**ARGS)
    lists, sens = tr.evaluate_sensitivity(**ARGS)
    assert lists == want and len(lists[0]) == 4
    assert tr.evaluate(**ARGS) == want                        # and evaluate is what it was afterwards
    _check(tr, lists, sens)
    again = tr.evaluate_sensitivity(**ARGS)[1]
    for pid in sens:                                          # deterministic
        np.testing.assert_array_equal(again[pid]["grads"], sens[pid]["grads"])
        np.testing.assert_array_equal(again[pid]["grads_abs"], sens[pid]["grads_abs"])
    # no per-policy filter: the default step is rel_step * 1.0; `steps` overrides, per policy id or index
    d = int(tr.cfg.obs_dim[0])
    by_id = tr.evaluate_sensitivity(steps={pid: np.full(d, 0.1) for pid in tr.policy_ids}, **ARGS)[1]
    by_ix = tr.evaluate_sensitivity(rel_step=0.5, steps=[np.full(d, 0.1)] * len(tr.policy_ids), **ARGS)[1]
    half = tr.evaluate_sensitivity(rel_step=0.05, **ARGS)[1]
    for pid in sens:
        np.testing.assert_array_equal(by_id[pid]["grads"], sens[pid]["grads"])
        np.testing.assert_array_equal(by_ix[pid]["grads_abs"], sens[pid]["grads_abs"])
        assert not np.array_equal(half[pid]["grads"], sens[pid]["grads"])
        assert half[pid]["grads_abs"].sum() < 0.75 * sens[pid]["grads_abs"].sum()
    with pytest.raises(ValueError, match="values"):
        tr.evaluate_sensitivity(steps=[np.full(3, 0.1)] * 4, **ARGS)
    tr.stop()


def test_default_steps_come_from_the_policy_filter():
    from ddrl_amd.trainer import PPOTrainer
    tr = PPOTrainer({**CFG, "observation_filter": "MeanStdFilter"}, n_envs=16, seed=3)
    rng = np.random.default_rng(5)
    d = int(tr.cfg.obs_dim[0])
    stats = [(500.0, rng.normal(size=d) * 0.2, np.abs(rng.normal(size=d)) * 499 + 5) for _ in tr.policy_ids]
    for p, st in enumerate(stats):
        tr.ctx.policy_filter_set(p, *st)
    lists, sens = tr.evaluate_sensitivity(**ARGS)
    _check(tr, lists, sens)
    explicit = tr.evaluate_sensitivity(steps=[0.1 * np.sqrt(S / (n - 1)) for n, M, S in stats], **ARGS)[1]
    for pid in sens:
        np.testing.assert_array_equal(explicit[pid]["grads"], sens[pid]["grads"])
    tr.stop()


def test_rollout_episodes_compute_gradient_writes_the_reference_files(tmp_path):
    from ddrl_amd.trainer import PPOTrainer
    tr = PPOTrainer(CFG, n_envs=16, seed=3)
    out = str(tmp_path / "grads")
    lists = evaluation.rollout_episodes_compute_gradient(None, tr, num_episodes=4, num_steps=20, experiment_nr=7,
                                                         out_dir=out, n_envs=2, seed=3)
    assert lists == tr.evaluate(**ARGS)
    d, A = int(tr.cfg.obs_dim[0]), tr.cfg.act_dim
    sens = tr.evaluate_sensitivity(**ARGS)[1]
    names = ["grads_tvel1_7.npy", "grads_tvel1_abs_7.npy"]
    for pid in tr.policy_ids:
        names += [f"grads_tvel1_7_{pid}.npy", f"grads_tvel1_abs_7_{pid}.npy"]
    assert sorted(os.listdir(out)) == sorted(names)
    first = tr.policy_ids[0]
    np.testing.assert_array_equal(np.load(os.path.join(out, "grads_tvel1_7.npy")), sens[first]["grads"])
    np.testing.assert_array_equal(np.load(os.path.join(out, "grads_tvel1_abs_7.npy")), sens[first]["grads_abs"])
    for pid in tr.policy_ids:
        g = np.load(os.path.join(out, f"grads_tvel1_7_{pid}.npy"))
        ga = np.load(os.path.join(out, f"grads_tvel1_abs_7_{pid}.npy"))
        assert g.shape == ga.shape == (d, A) and g.dtype == np.float64
        np.testing.assert_array_equal(ga, sens[pid]["grads_abs"])
        # as the plot normalizes them: every action column sums to 1
        np.testing.assert_allclose((ga / ga.sum(0)).sum(0), 1.0, rtol=1e-12)
    with pytest.raises(NotImplementedError):
        evaluation.rollout_episodes_compute_gradient(None, tr, render=True)
    tr.stop()
