"""PopulationTrainer: the seeds of one experiment trained side by side, their update launches of an
iteration replaced by one group launch.  Member m is the solo PPOTrainer of seed m bit for bit:
weights, Adam state, KL coefficients, filters and learner statistics after two iterations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEEDS = (0, 1, 2)
CONFIG = {"env": "QuantrupedMultiEnv_Local", "rollout_fragment_length": 32, "num_sgd_iter": 2}
# timings differ between any two runs; everything else of a result is compared
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
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


def _trainer_state(t):
    out = {"weights": t.get_weights(), "kl": list(t.kl_coeff), "filter": list(t.ctx.filter_get()),
           "iteration": t.iteration, "timesteps": t.timesteps_total}
    for p in range(t.cfg.n_policies):
        out[f"adam{p}"] = list(t.ctx.adam_get(p))
    return out


def test_population_matches_solo_trainers(tmp_path):
    from ddrl_amd.population import PopulationTrainer
    from ddrl_amd.trainer import PPOTrainer
    pop = PopulationTrainer(CONFIG, SEEDS, n_envs=8)
    assert [t.cfg.n_envs for t in pop.trainers] == [8, 8, 8]
    pop_results = [pop.train() for _ in range(2)]
    pop_state = [_trainer_state(t) for t in pop.trainers]
    # each launch's chains sat on one XCD each: 3 members x 4 policies in one launch
    xcc = pop.group.placement()
    assert xcc.size == 32 + 24 + 4
    paths = pop.save(str(tmp_path))
    assert len(paths) == 3
    for m, s in enumerate(SEEDS):
        solo = PPOTrainer(CONFIG, n_envs=8, seed=s)
        for it in range(2):
            r = solo.train()
            g = pop_results[it][m]
            _same(UNTIMED(g), UNTIMED(r), f"seed {s} iteration {it}")
            assert set(g["info"]["learner"]) == set(solo.policy_ids)
        _same(pop_state[m], _trainer_state(solo), f"seed {s} state")
        solo.stop()
    # restore puts every member's checkpoint back
    w0 = pop.trainers[0].get_weights()
    pop.train()
    pop.restore(str(tmp_path))
    _same(pop.trainers[0].get_weights(), w0, "restored weights")
    pop.stop()
    assert pop.trainers == [] and pop.group is None


def test_population_refuses_what_the_group_refuses():
    from ddrl_amd.native import DdrlError
    from ddrl_amd.population import PopulationTrainer
    from tests.gpu_harness import GNN_ENV
    with pytest.raises(DdrlError, match="member 0 is a GraphNet context"):
        PopulationTrainer({**CONFIG, "env": GNN_ENV}, (0, 1), n_envs=8)
    with pytest.raises(DdrlError, match="sgd_minibatch_size 256"):
        PopulationTrainer({**CONFIG, "sgd_minibatch_size": 256}, (0, 1), n_envs=8)
    with pytest.raises(ValueError, match="single-process replicas"):
        PopulationTrainer({**CONFIG, "parallel": "gather"}, (0, 1), n_envs=8)
