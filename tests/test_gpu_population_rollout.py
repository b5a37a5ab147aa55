"""PopulationTrainer on the device env plane: the members' fragments of an iteration as one group
chain (native.RolloutGroup) besides the one group update.  Member m stays the solo PPOTrainer of
seed m bit for bit -- results, weights, Adam state, KL coefficients and filters after two
iterations -- and equals the same population sampling member by member (needs an MI355X)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEEDS = (0, 1, 2)
CONFIG = {"env": "QuantrupedMultiEnv_Local", "env_backend": "device", "rollout_fragment_length": 32, "num_sgd_iter": 2}
UNEVEN = {**CONFIG, "env_config": {"hf_smoothness": 0.8}}
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
           "env_state": t.backend.env.state(), "iteration": t.iteration, "timesteps": t.timesteps_total}
    for p in range(t.cfg.n_policies):
        out[f"adam{p}"] = list(t.ctx.adam_get(p))
        if t.cfg.policy_filter:
            out[f"pfilter{p}"] = list(t.ctx.policy_filter_get(p))
    return out


def _population(config, group_rollout):
    from ddrl_amd.population import PopulationTrainer
    pop = PopulationTrainer(config, SEEDS, n_envs=8, group_rollout=group_rollout)
    assert (pop.rollout_group is not None) == (group_rollout is not False)
    results = [pop.train() for _ in range(2)]
    state = [_trainer_state(t) for t in pop.trainers]
    pop.stop()
    assert pop.trainers == [] and pop.group is None and pop.rollout_group is None
    return results, state


@pytest.mark.parametrize("config", [CONFIG, UNEVEN], ids=["flat", "uneven"])
def test_group_rollout_matches_solo_trainers_and_member_sampling(config):
    from ddrl_amd.trainer import PPOTrainer
    grp_results, grp_state = _population(config, None)        # None: the device plane selects the group rollout
    seq_results, seq_state = _population(config, False)
    for m, s in enumerate(SEEDS):
        solo = PPOTrainer(config, n_envs=8, seed=s)
        for it in range(2):
            r = UNTIMED(solo.train())
            _same(UNTIMED(grp_results[it][m]), r, f"group rollout, seed {s} iteration {it}")
            _same(UNTIMED(seq_results[it][m]), r, f"member sampling, seed {s} iteration {it}")
        st = _trainer_state(solo)
        _same(grp_state[m], st, f"group rollout, seed {s} state")
        _same(seq_state[m], st, f"member sampling, seed {s} state")
        solo.stop()
    # the runs were not trivially equal: the seeds differ from each other
    assert not np.array_equal(grp_state[0]["env_state"], grp_state[1]["env_state"])


def test_group_rollout_with_the_policy_filter():
    """explicit True, per-policy MeanStdFilter on: against the member-by-member population."""
    config = {**CONFIG, "observation_filter": "MeanStdFilter"}
    grp_results, grp_state = _population(config, True)
    seq_results, seq_state = _population(config, False)
    for it in range(2):
        for m in range(len(SEEDS)):
            _same(UNTIMED(grp_results[it][m]), UNTIMED(seq_results[it][m]), f"member {m} iteration {it}")
    _same(grp_state, seq_state, "state")


def test_synthetic_plane_falls_back_or_refuses():
    from ddrl_amd.population import PopulationTrainer
    synthetic = {k: v for k, v in CONFIG.items() if k != "env_backend"}
    with pytest.raises(ValueError, match="group_rollout needs every member on the device env plane"):
        PopulationTrainer(synthetic, (0, 1), n_envs=8, group_rollout=True)
    pop = PopulationTrainer(synthetic, (0, 1), n_envs=8)       # None: member by member
    assert pop.rollout_group is None
    r = pop.train()
    assert len(r) == 2 and all(x["timesteps_total"] == 8 * 32 for x in r)
    pop.stop()
    assert pop.trainers == [] and pop.group is None and pop.rollout_group is None
