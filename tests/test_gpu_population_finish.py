"""PopulationTrainer with the members' finish -- GAE and the episode accounting -- as one group chain
(native.FinishGroup) and the learner statistics read in one call (UpdateGroup.stats_range): member m
stays the solo PPOTrainer of seed m bit for bit -- result dicts without the timers, weights and
checkpoint files after two iterations -- and equals the same population finishing member by member.
Planes: the device env plane (with the group rollout) and the synthetic plane sampled member by
member.  Three seeds, 8 envs, T = 16 (needs an MI355X)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEEDS = (0, 1, 2)
SYNTHETIC = {"env": "QuantrupedMultiEnv_Local", "rollout_fragment_length": 16, "num_sgd_iter": 2}
DEVICE = {**SYNTHETIC, "env_backend": "device"}
UNTIMED = lambda r: {k: v for k, v in r.items() if k != "timers"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same(a, b, what):
    """Bitwise equality of nested results (NaN == NaN: an iteration without finished episodes)."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), f"{what}: keys {list(a)} != {list(b)}"
        for k in a:
            _same(a[k], b[k], f"{what}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        assert type(a) is type(b), (what, type(a), type(b))
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


def _npz(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _population(config, group_finish, group_rollout, directory):
    from ddrl_amd.population import PopulationTrainer
    pop = PopulationTrainer(config, SEEDS, n_envs=8, group_rollout=group_rollout, group_finish=group_finish)
    assert (pop.finish_group is not None) == (group_finish is not False)
    results = [pop.train() for _ in range(2)]
    weights = [t.get_weights() for t in pop.trainers]
    files = [_npz(p) for p in pop.save(directory)]
    pop.stop()
    assert pop.trainers == [] and pop.group is None and pop.finish_group is None
    return results, weights, files


@pytest.mark.parametrize("config,group_rollout", [(DEVICE, None), (SYNTHETIC, False)], ids=["device", "synthetic"])
def test_group_finish_matches_member_finish_and_solo_trainers(config, group_rollout, tmp_path):
    from ddrl_amd.trainer import PPOTrainer
    runs = {name: _population(config, gf, group_rollout, str(tmp_path / name))
            for name, gf in (("default", None), ("group", True), ("members", False))}
    for m, s in enumerate(SEEDS):
        solo = PPOTrainer(config, n_envs=8, seed=s)
        results = [UNTIMED(solo.train()) for _ in range(2)]
        weights = solo.get_weights()
        saved = _npz(solo.save(os.path.join(str(tmp_path), "solo", f"seed_{s}.npz")))
        solo.stop()
        for name, (r, w, f) in runs.items():
            for it in range(2):
                _same(UNTIMED(r[it][m]), results[it], f"{name}, seed {s} iteration {it}")
            _same(w[m], weights, f"{name}, seed {s} weights")
            _same(f[m], saved, f"{name}, seed {s} checkpoint")
    # the runs were not trivially equal: the seeds differ from each other, and the learner trained
    group = runs["group"]
    assert not np.array_equal(next(iter(group[1][0].values())), next(iter(group[1][1].values())))
    assert all(np.isfinite(v) for r in group[0][1] for st in r["info"]["learner"].values() for v in st.values())
