"""PPOTrainer.evaluate / compute_action and ddrl_amd.evaluation over the device path: the
reference's evaluation surface (evaluation/rollout_episodes.py:26-164,
evaluation/evaluate_trained_policies_pd.py:84-127) for a trainer and for the published Local
policies (tests/golden/ckpt_local_1250.npz)."""
import json
import os

import numpy as np
import pytest

from ddrl_amd import evaluation, native as N
from oracle import ddrl_oracle as O
from tests import eval_reference as R
from tests.gpu_harness import OracleRollout

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_local_1250.npz")
CFG = {"env": "QuantrupedMultiEnv_Local", "rollout_fragment_length": 8}


def _check_tuple(res, n, num_steps):
    assert len(res) == 6 and all(isinstance(col, list) and len(col) == n for col in res)
    reward, steps, dist, power, vel, cot = (np.asarray(c, np.float64) for c in res)
    assert np.isfinite(reward).all() and np.isfinite(dist).all() and np.isfinite(power).all()
    assert all(isinstance(s, int) for s in res[1]) and steps.min() >= 1 and steps.max() <= num_steps
    np.testing.assert_array_equal(vel, dist / steps)
    with np.errstate(divide="ignore", invalid="ignore"):
        np.testing.assert_array_equal(cot, (power / steps) / (N.TOTAL_MASS * vel))
    assert (power > 0).all()


def test_trainer_evaluate_and_training_is_untouched():
    from ddrl_amd.trainer import PPOTrainer
    tr = PPOTrainer(CFG, n_envs=16, seed=3)
    twin = PPOTrainer(CFG, n_envs=16, seed=3)
    args = dict(num_episodes=6, num_steps=25, explore=False, n_envs=4, env_filter="frozen")
    res = tr.evaluate(**args)
    _check_tuple(res, 6, 25)
    assert tr.evaluate(**args) == res                       # frozen filter, same seed: the same lists
    assert evaluation.rollout_episodes(None, tr, num_episodes=6, num_steps=25, explore_during_rollout=False,
                                       n_envs=4, env_filter="frozen") == res
    with pytest.raises(NotImplementedError):
        evaluation.rollout_episodes(None, tr, render=True)
    # the default samples (the reference's compute_action call passes no `explore`), other filter modes run
    res_x = tr.evaluate(num_episodes=5, num_steps=20, n_envs=4)
    _check_tuple(res_x, 5, 20)
    assert res_x[0] != res[0][:5]
    _check_tuple(tr.evaluate(num_episodes=3, num_steps=10, n_envs=3, env_filter="fresh", explore=False), 3, 10)
    with pytest.raises(ValueError, match="env_filter"):
        tr.evaluate(env_filter="other")
    # training after evaluation: the result and the weights of a twin that never evaluated
    ra, rb = tr.train(), twin.train()
    for pid, st in ra["info"]["learner"].items():
        for k, v in st.items():
            np.testing.assert_array_equal(v, rb["info"]["learner"][pid][k], err_msg=f"{pid} {k}")
    assert {k: ra[k] for k in ("training_iteration", "timesteps_total")} == \
        {k: rb[k] for k in ("training_iteration", "timesteps_total")}
    for pid, w in tr.get_weights().items():
        np.testing.assert_array_equal(w, twin.get_weights()[pid])
    np.testing.assert_array_equal(tr.ctx.filter_get()[1], twin.ctx.filter_get()[1])
    # compute_action: one row through ddrl_eval_act's logits
    p = 1
    d, A = int(tr.cfg.obs_dim[p]), tr.cfg.act_dim
    x = np.random.default_rng(0).normal(size=d).astype(np.float32)
    prm = O.unpack(tr.ctx.params_get(p), O.ffn_param_shapes(d, 2 * A))
    logits = O.ffn_forward(prm, x[None])[0][0]
    a = tr.compute_action(x, tr.policy_ids[p], explore=False)
    assert a.shape == (A,)
    np.testing.assert_allclose(a, np.clip(logits[:A], -1, 1), rtol=1e-5, atol=2e-5)
    assert not np.array_equal(tr.compute_action(x, tr.policy_ids[p], seed=1), a)
    tr.stop()
    twin.stop()


def test_published_local_policies_evaluate():
    """The published Local policies: finite rows, and the first step's actions of the evaluation
    loop match the deterministic oracle at the rollout parity tolerance."""
    import torch
    from ddrl_amd.trainer import PPOTrainer
    z = np.load(FIX, allow_pickle=False)
    pids = json.loads(bytes(z["policy_ids"]).decode())
    states = {pid: {"weights": z[f"{pid}/weights"], "adam_m": z[f"{pid}/adam_m"], "adam_v": z[f"{pid}/adam_v"],
                    "beta_powers": tuple(float(x) for x in z[f"{pid}/beta_powers"]),
                    "filter": (float(z[f"{pid}/filter_n"][0]), z[f"{pid}/filter_M"], z[f"{pid}/filter_S"]),
                    "kl_coeff": float(z[f"{pid}/kl_coeff"][0])} for pid in pids}
    tr = PPOTrainer({**CFG, "observation_filter": "MeanStdFilter"}, n_envs=16, seed=2)
    tr.load_policy_states(states)
    res = tr.evaluate(num_episodes=8, num_steps=30, explore=False, n_envs=4, env_filter="frozen", seed=5)
    _check_tuple(res, 8, 30)
    rows = [dict(zip(evaluation.COLUMNS[5:], r)) for r in zip(*res)]
    assert set(rows[0]) == {"reward", "duration", "distance", "power", "velocity", "CoT"}

    # the first step of that loop, issued by hand on the evaluation context against the oracle
    n = 4
    ectx = tr._eval_context(n)
    cfg = ectx.cfg
    filt = tr.rctx.filter_get()
    ectx.filter_set(*filt)
    env = N.HostEnv(n, 43, n_threads=1, seed=5)
    obs = env.reset_episodes()
    shapes = O.ffn_param_shapes(35, 4)
    orc = OracleRollout(cfg, tr.env, [O.unpack(states[pid]["weights"], shapes) for pid in tr.policy_ids], filt)
    for p, pid in enumerate(tr.policy_ids):
        orc.pf[p].n, orc.pf[p].M[:], orc.pf[p].S[:] = states[pid]["filter"]
    actions = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    ectx.eval_begin(1, filter_update=False)
    ectx.eval_act(torch.from_numpy(obs).cuda(), None, actions)
    ectx.synchronize()
    ectx.eval_end()
    R.eval_observe(orc, obs, filter_update=False)
    a_orc, _ = R.eval_act(orc, None)
    np.testing.assert_allclose(actions.cpu().numpy(), a_orc, rtol=1e-5, atol=2e-5)
    env.close()
    tr.stop()


def test_write_csv_has_the_reference_columns(tmp_path):
    rows = [{"approach": "Local", "seed": 0, "trained_on": "flat", "evaluated_on": 1.0, "simulation_run": i,
             "reward": 1.0 * i, "duration": 10, "distance": 0.5, "power": 2.0, "velocity": 0.05, "CoT": 4.5}
            for i in range(3)]
    path = evaluation.write_csv(rows, str(tmp_path / "evaluation_1.0.csv"))
    lines = open(path).read().splitlines()
    assert lines[0] == "approach,seed,trained_on,evaluated_on,simulation_run,reward,duration,distance,power,velocity,CoT"
    assert len(lines) == 4 and lines[2].startswith("Local,0,flat,1.0,1,1.0,10,")
