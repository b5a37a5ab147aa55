"""fp64 / fp32 numpy restatement of the input-sensitivity evaluation, for the sensitivity tests.

Written from the arithmetic of the reference's evaluation/rollout_episodes_compute_gradient.py:
  :62-66    step_dim_low / high = -+0.1 * rs.std[i] of the policy's MeanStdFilter
  :114-120  2 d compute_action(explore=False) calls on the observation moved in one dimension
  :121-122  manual_grads += act_high - act_low; manual_grads_abs += |act_high - act_low|
with the library's semantics: the step h_f is added to the env-normalized input in fp64 (the
arithmetic of tests/eval_reference.eval_observe), before the per-policy filter and the rounding
to fp32; constant inputs (the LegID one-hot) are not moved; the clipped means are float32 and
subtracted in float32, the sums are fp64; an env counts while it is below its episode quota.
"""
import numpy as np

from oracle import ddrl_oracle as O


T = 3
TVEL = {"env_config": {"target_velocity": [1.0]}}
PFILTER = {"observation_filter": "MeanStdFilter"}
CUP_ENV = "QuantrupedMultiEnv_SharedDecentralLegID"
CUP_CONFIG = {"model": {"custom_model": "cup"}}

# name -> (env, n, config, workgroups per policy or None).  With a cap the workgroups loop over
# base rows: 12 rows over 5 workgroups is 3, 3, 2, 2, 2 (a ragged last pass), 3 rows over 2 is 2, 1.
CASES = {
    "central_tvel3": ("QuantrupedMultiEnv_Centralized", 3, TVEL, None),   # d = 44, A = 8: 88 rows, last tile half full
    "central_tvel3_loop": ("QuantrupedMultiEnv_Centralized", 3, TVEL, 2),
    "local5_pfilter": ("QuantrupedMultiEnv_Local", 5, PFILTER, None),     # 4 policies, d = 35: 70 rows
    "shared3": ("QuantrupedMultiEnv_SharedDecentral", 3, None, None),     # k = 4: 12 base rows, d = 19
    "shared3_loop": ("QuantrupedMultiEnv_SharedDecentral", 3, None, 5),
    "twosides2": ("QuantrupedMultiEnv_TwoSides", 2, None, None),          # A = 4
    "cup3": (CUP_ENV, 3, CUP_CONFIG, None),                               # coupling applied
    "legid3": (CUP_ENV, 3, None, None),                                   # d = 23: four constant inputs per row
}
# the oracle test runs with the per-policy filter wherever the model has no constant input
ORACLE_CASES = {k: (e, n, ({**(c or {}), **PFILTER} if k != "legid3" else c), g) for k, (e, n, c, g) in CASES.items()}


def is_cup(config):
    return bool(config and (config.get("model") or {}).get("custom_model") == "cup")


def filt(D, rng):
    return 100.0, rng.normal(size=D) * 0.1, np.abs(rng.normal(size=D)) * 99 + 1


def pfilt(cfg, rng):
    return [(500.0, rng.normal(size=cfg.obs_dim[p]) * 0.2, np.abs(rng.normal(size=cfg.obs_dim[p])) * 499 + 5)
            for p in range(cfg.n_policies)]


def oracle_case(name):
    """The seeded inputs of the oracle test (tests/test_gpu_sens.py), shared with the CPU test of the
    bars they must meet: (cfg, inst, config, filt, pfilt, obs, steps)."""
    from ddrl_amd.spec import make_cfg
    from tests.gpu_harness import synthetic_inputs
    env, n, config, _ = ORACLE_CASES[name]
    cfg, inst = make_cfg(env, n, T, config)
    rng = np.random.default_rng(31)
    f = filt(cfg.obs_full_dim, rng)
    obs = synthetic_inputs(rng, cfg, T)[0]
    pf = pfilt(cfg, rng) if cfg.policy_filter else None
    steps = ([default_steps(n_, S_, M_) for n_, M_, S_ in pf] if pf
             else [np.full(cfg.obs_dim[p], 0.1) for p in range(cfg.n_policies)])
    return cfg, inst, config, f, pf, obs, steps


def make_oracle(cfg, inst, config, params, f, pf):
    from tests.gpu_harness import CupOracleRollout, OracleRollout
    orc = (CupOracleRollout if is_cup(config) else OracleRollout)(cfg, inst, params, f)
    for p, st in enumerate(pf or []):
        orc.pf[p].n, orc.pf[p].M[:], orc.pf[p].S[:] = st
    return orc


def default_steps(n, S, M=None, rel_step=0.1):
    """rel_step * rs.std of a RunningStat (n, M, S): sqrt(S / (n - 1)), |M| while n <= 1."""
    rs = O.RunningStat(np.shape(S))
    rs.n, rs.S[...] = n, S
    if M is not None:
        rs.M[...] = M
    return rel_step * rs.std


def perturbed_inputs(orc, obs, steps, filter_update=False):
    """Per policy: (x [2d, C, d] float32, base [C, d] float32, moved [k, d] bool).  x[2f] is the base
    input with feature f built from z_f - h_f, x[2f + 1] from z_f + h_f (c = env * k + slot);
    moved[slot, f] is False for constant inputs, whose two rows equal the base row."""
    cfg = orc.cfg
    normed = O.mean_std_filter(obs, orc.rs, update=bool(filter_update), clip=cfg.filter_clip)
    tables = orc.model_tables()
    n = normed.shape[0]
    ext = np.concatenate([normed, np.zeros((n, 1)), np.ones((n, 1))], 1)
    col = lambda i: i if i >= 0 else normed.shape[1] + (-1 - i)
    out = []
    for p in range(cfg.n_policies):
        d, k = cfg.obs_dim[p], len(orc.slots[p])
        z = np.stack([ext[:, [col(i) for i in tables[a]]] for a in orc.slots[p]], 1)   # [n, k, d] fp64
        moved = np.array([[i >= 0 for i in tables[a]] for a in orc.slots[p]])          # [k, d]
        h = np.asarray(steps[p], np.float64)

        def finish(zz):
            x = zz.reshape(-1, d)
            if orc.pf is not None:
                x = O.mean_std_filter(x, orc.pf[p], update=False, clip=None)
            return x.astype(np.float32)

        x = np.empty((2 * d, n * k, d), np.float32)
        for f in range(d):
            for sign, r in ((-1.0, 2 * f), (1.0, 2 * f + 1)):
                zz = z.copy()
                zz[:, :, f] = np.where(moved[:, f], z[:, :, f] + sign * h[f], z[:, :, f])
                x[r] = finish(zz)
        out.append((x, finish(z), moved))
    return out


def sens_means(orc, obs, steps, filter_update=False):
    """Per policy: (means [C, 2d, A] float32 -- the clipped action means of the perturbed rows, NaN
    where the input is constant --, base means [C, A], moved [k, d])."""
    cfg = orc.cfg
    A = cfg.act_dim
    res = []
    for p, (x, base, moved) in enumerate(perturbed_inputs(orc, obs, steps, filter_update)):
        d, k = cfg.obs_dim[p], len(orc.slots[p])
        C = base.shape[0]
        means = np.empty((C, 2 * d, A), np.float32)
        for r in range(2 * d):   # one forward per perturbed row index: row c of the batch is base row c
            means[:, r] = np.clip(orc.forward(p, x[r])[0][:, :A], -1.0, 1.0)
            means[~np.tile(moved[:, r >> 1], C // k), r] = np.nan
        res.append((means, np.clip(orc.forward(p, base)[0][:, :A], -1.0, 1.0), moved))
    return res


def terms(means):
    """The fp32 differences [C, d, A] of a means block [C, 2d, A]; 0 where the input is constant."""
    diff = means[:, 1::2].astype(np.float32) - means[:, 0::2].astype(np.float32)
    return np.where(np.isnan(diff), np.float32(0), diff)


class SensAccumulator:
    """grads / grads_abs [d, A] (fp64) and the accumulated base rows per policy."""

    def __init__(self, cfg):
        self.cfg = cfg
        A = cfg.act_dim
        self.grads = [np.zeros((cfg.obs_dim[p], A)) for p in range(cfg.n_policies)]
        self.grads_abs = [np.zeros((cfg.obs_dim[p], A)) for p in range(cfg.n_policies)]
        self.mag = [np.zeros((cfg.obs_dim[p], A)) for p in range(cfg.n_policies)]   # sum of |terms| (bounds)
        self.rows = [0] * cfg.n_policies

    def step(self, means, env_open=None):
        """means: per policy [C, 2d, A]; env_open [N] bool: the envs below their quota (None: all)."""
        for p, m in enumerate(means):
            k = m.shape[0] // self.cfg.n_envs
            keep = np.ones(m.shape[0], bool) if env_open is None else np.repeat(np.asarray(env_open, bool), k)
            t = terms(m)[keep].astype(np.float64)
            self.grads[p] += t.sum(0)
            self.grads_abs[p] += np.abs(t).sum(0)
            self.mag[p] += np.abs(t).sum(0)
            self.rows[p] += int(keep.sum())


def fd_matrix(forward, x, h):
    """The reference matrix of one row for a plain function: [d, A] with entry (f, j) =
    forward(x + h_f e_f)[j] - forward(x - h_f e_f)[j], in fp64."""
    x = np.asarray(x, np.float64)
    out = []
    for f in range(x.size):
        e = np.zeros_like(x)
        e[f] = h[f]
        out.append(np.asarray(forward(x + e), np.float64) - np.asarray(forward(x - e), np.float64))
    return np.stack(out)
