"""PPO trainer over the HIP hot path -- the drop-in for train_experiment_1's tune.run("PPO").

Reference call stack: RLlib PPOTrainer with ParallelRollouts ->
postprocess_ppo_gae -> StandardizeFields(["advantages"]) -> TrainTFMultiGPU (num_sgd_iter
epochs over R // sgd_minibatch_size shuffled minibatches per policy) -> update_kl.
Here one `train()` call is one training iteration: T = rollout_fragment_length vector env
steps on the device, bootstrap + GAE on the device, then one fused persistent update launch
for all policies (or, for a shared policy across ranks, per-minibatch gradient all-reduce).

The config dict uses the reference's keys (train_experiment_1_architecture_on_flat.py:96-168).
"""
from __future__ import annotations

import json
import math
import os
import time

import numpy as np

from . import native as N
from .metrics import EpisodeHistory, ProgressLogger, gather_rank_rows
from .spec import PPO_DEFAULTS, make_cfg


def glorot_ffn_flat(rng, d, A, hidden=64):
    """GlorotUniformScaled init (models/glorot_uniform_scaled_initializer.py:3-19): hidden
    kernels scale 1.0, fc_out / value_out scale 0.01, biases 0; Keras flat order."""
    def g(fi, fo, s):
        lim = math.sqrt(6.0 * s / (fi + fo))
        return rng.uniform(-lim, lim, size=(fi, fo)).astype(np.float32)
    z = lambda n: np.zeros(n, np.float32)
    parts = [g(d, hidden, 1.0), z(hidden), g(d, hidden, 1.0), z(hidden),
             g(hidden, hidden, 1.0), z(hidden), g(hidden, hidden, 1.0), z(hidden),
             g(hidden, 2 * A, 0.01), z(2 * A), g(hidden, 1, 0.01), z(1)]
    return np.concatenate([p.reshape(-1) for p in parts])


def leg_coupling_init(A):
    """LegCoupling.build (models/coupling_net_glorot_uniform_init.py:20): the table starts at
    [[1, 1], [-1, -1], [-1, -1], [1, 1]] (FL, HL, HR, FR), not at a random draw."""
    return np.resize(np.array([[1, 1], [-1, -1], [-1, -1], [1, 1]], np.float32), (4, A)).reshape(-1)


def rank_seeds(seed, rank):
    """(env seed, exploration-noise seed) of one rank: every rank samples its own trajectories
    (like RLlib's rollout workers, whose envs are seeded per worker index), while the weights
    come from `seed` alone and are identical on every rank.  Rank 0 keeps the single-process
    seeds."""
    return seed + 1_000_003 * rank, seed + 1 + 1_000_003 * rank


_warned_synthetic_terrain = False


def _warn_synthetic_terrain():
    """Once per process: the synthetic backend draws its observations and has no ground."""
    global _warned_synthetic_terrain
    if not _warned_synthetic_terrain:
        import warnings
        _warned_synthetic_terrain = True
        warnings.warn("env_config hf_smoothness < 1 has no effect on the synthetic env backend (it has no "
                      "terrain): use env_backend 'host' or 'device' to train on uneven ground", stacklevel=3)


class PPOTrainer:
    """Multi-agent PPO on one device (one env shard).

    env_backend: an object with reset() -> obs[N, D] (device tensor) and
    step(actions[N, 8]) -> (obs_next, fw[N], cfrc[N, 14, 6], done[N] uint8); defaults to the
    synthetic vectorized QuAntruped (`ddrl_amd.envs.SyntheticVecEnv`).
    """

    def __init__(self, config, n_envs=None, device=0, env_backend=None, seed=0, stream=None):
        """Multi-process use: initialize torch.distributed first (one process per GPU).
        Shared-policy envs then train data-parallel (config "parallel": "ddp", the default
        for one policy; "ddp_mode": "split" | "local", see ddrl_amd.ddp); multi-policy envs
        run as independent replicas ("parallel": "replicas").  "parallel": "gather" (any env):
        every rank rolls out its own envs, the records of all ranks are all-gathered once per
        iteration into a learner context sized for the union batch, and every rank runs the
        same fused update over it with the same schedule -- weights identical on all ranks, no
        per-step collective (the union batch equals a single-process run over all envs)."""
        import torch
        import torch.distributed as dist
        self.torch = torch
        self.config = {**PPO_DEFAULTS, **config}
        c = self.config
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        env = c["env"]
        self.n_envs = int(n_envs or c.get("num_envs", c.get("num_workers", 2) * c.get("num_envs_per_worker", 4)))
        self.T = int(c["rollout_fragment_length"])
        self.cfg, self.env = make_cfg(env, self.n_envs, self.T, c)
        self.parallel = c.get("parallel") or ("ddp" if self.world > 1 and self.cfg.n_policies == 1 else "replicas")
        if self.parallel not in ("ddp", "replicas", "gather"):
            raise ValueError(f"parallel {self.parallel!r}: 'ddp', 'replicas' or 'gather'")
        # extension: "rng_backend": "device" draws the exploration noise and the minibatch schedules
        # on the device from a counter-based generator (csrc/rng.hip) instead of torch / numpy on the
        # host; "host" (the default) is the path as it always was
        self.rng_backend = c.get("rng_backend", "host")
        if self.rng_backend not in ("host", "device"):
            raise ValueError(f"rng_backend {self.rng_backend!r}: 'host' or 'device'")
        if self.rng_backend == "device" and self.parallel == "ddp":
            raise ValueError("rng_backend 'device' does not cover parallel 'ddp': its learners draw their own "
                             "schedule on the host; use rng_backend 'host', or parallel 'replicas' / 'gather'")
        torch.cuda.set_device(device)
        self.device = torch.device("cuda", device)
        self.stream = stream or torch.cuda.current_stream(self.device)
        self.ctx = N.Context(self.cfg, device, self.stream.cuda_stream)
        self.policy_ids = list(type(self.env).policy_names)
        P = self.cfg.n_policies
        self.rng = np.random.default_rng(seed)              # weights: identical on every rank
        self.sched_rng = np.random.default_rng(seed + 7919 * (self.rank + 1))
        env_seed, noise_seed = rank_seeds(seed, self.rank)  # trajectories: different on every rank
        for p in range(P):
            if self.cfg.model_kind == N.MODEL_FFN:
                theta = glorot_ffn_flat(self.rng, self.cfg.obs_dim[p], self.cfg.act_dim)
                if self.cfg.leg_coupling:
                    theta = np.concatenate([theta, leg_coupling_init(self.cfg.act_dim)])
                self.ctx.params_set(p, theta)
            else:
                from .models import glorot_gnn_flat
                layer = {v: k for k, v in N.GNN_LAYERS.items()}[self.cfg.gnn_layer]
                self.ctx.params_set(p, glorot_gnn_flat(self.rng, self.cfg.act_dim, layer=layer))
        self.kl_coeff = [float(c["kl_coeff"])] * P
        # the ground of the env planes: env_config["hf_smoothness"] (1.0: flat) and the curriculum
        # keys of the adaptor (curriculum_learning, range_smoothness, range_last_timestep)
        self.hf_smoothness = float(getattr(self.env, "hf_smoothness", 1.0))
        if env_backend is None and c.get("env_backend", "synthetic") == "host":
            # extension: the host env plane (the QuAntruped stand-in on host threads; TVel
            # target velocities drawn per env from env_config["target_velocity"] on every reset)
            from .envs import HostVecEnv, curriculum_of
            env_backend = HostVecEnv(self.n_envs, self.cfg.obs_full_dim, self.device, seed=env_seed,
                                     n_threads=int(c.get("num_host_threads", 4)),
                                     target_velocity=self.env.target_velocity_list or 0.0,
                                     hf_smoothness=self.hf_smoothness, curriculum=curriculum_of(getattr(self.env, "config", {})))
        elif env_backend is None and c.get("env_backend", "synthetic") == "device":
            # extension: the device env plane (the same stand-in stepped by a HIP kernel on the
            # rollout context's stream: no host threads, no copies)
            from .envs import DeviceVecEnv, curriculum_of
            env_backend = DeviceVecEnv(self.ctx, seed=env_seed, target_velocity=self.env.target_velocity_list or 0.0,
                                       hf_smoothness=self.hf_smoothness, curriculum=curriculum_of(getattr(self.env, "config", {})))
        elif env_backend is None:
            from .envs import SyntheticVecEnv
            if self.hf_smoothness < 1.0:
                _warn_synthetic_terrain()
            env_backend = SyntheticVecEnv(self.n_envs, self.cfg.obs_full_dim, self.device, seed=env_seed)
        self.backend = env_backend
        self.actions = torch.zeros((self.n_envs, 8), dtype=torch.float32, device=self.device)
        self.noise_gen = torch.Generator(device=self.device)
        self.noise_gen.manual_seed(noise_seed)
        self.timesteps_total = 0
        self.iteration = 0
        self.rctx = self.ctx   # the rollout context (the learner's own, except in "gather" mode)
        self.episode_history = EpisodeHistory(int(c["metrics_smoothing_episodes"]))
        self.episodes_total = 0
        if self.parallel == "replicas" and self.world > 1:   # only the episode metrics cross the ranks
            from .ddp import Comm
            self.comm = Comm(self.device if dist.get_backend() == "nccl" else "cpu")
        if self.parallel == "gather":
            from .ddp import Comm
            self.comm = Comm(self.device if self.world > 1 and dist.get_backend() == "nccl" else "cpu") \
                if self.world > 1 else None
            ucfg, _ = make_cfg(env, self.n_envs * self.world, self.T, c)
            self.ctx = N.Context(ucfg, device, self.stream.cuda_stream)   # learner: union batch
            for p in range(P):
                self.ctx.params_set(p, self.rctx.params_get(p))
            self.pfilter_base = ([self.rctx.policy_filter_get(p) for p in range(P)]
                                 if self.cfg.policy_filter else None)
            self.rctx.policy_filter_delta_reset()
            self.sched_rng = np.random.default_rng(seed + 7919)   # the same schedule on every rank
        if self.rng_backend == "device":
            # the seeds of the host generators: noise_seed on the rollout context, sched_rng's on the learner
            self._init_device_rng(noise_seed, seed + 7919 * (1 if self.parallel == "gather" else self.rank + 1))
        if self.parallel == "ddp":
            from .ddp import (Comm, DataParallelLearner, HipBackend, NativeDataParallelLearner, PeerLearner,
                              native_comm_init)
            rccl = dist.get_backend() == "nccl"
            self.comm = Comm(self.device if rccl else "cpu")
            loop = c.get("ddp_loop", "native")
            if loop == "peer":
                # extension: the two ranks' update as one fused launch split across them; only for
                # what ddrl_peer_attach supports, otherwise the all-reduce learner
                why = [w for w, bad in (("a GraphNet model", self.cfg.model_kind != N.MODEL_FFN),
                                        (f"{self.world} ranks (peer mode pairs exactly two)", self.world != 2),
                                        (f"sgd_minibatch_size {self.cfg.sgd_minibatch_size} (not 128)",
                                         self.cfg.sgd_minibatch_size != 128),
                                        ("DDRL_UPDATE_SPLIT=1 (peer mode needs the row split)",
                                         os.environ.get("DDRL_UPDATE_SPLIT") == "1")) if bad]
                if why:
                    import warnings
                    warnings.warn(f"ddp_loop 'peer' does not support {', '.join(why)}: using the all-reduce "
                                  "data-parallel learner")
                    loop = "native" if rccl else "python"
            if loop == "peer":
                self.learner = PeerLearner(self.ctx, self.comm, 0, self.cfg.sgd_minibatch_size)
            elif rccl and loop == "native":
                native_comm_init(self.ctx, self.comm)
                self.learner = NativeDataParallelLearner(self.ctx, self.comm, 0, self.cfg.sgd_minibatch_size,
                                                         c.get("ddp_mode", "split"))
            else:
                self.learner = DataParallelLearner(HipBackend(self.ctx), self.comm, 0, self.cfg.sgd_minibatch_size,
                                                   c.get("ddp_mode", "split"))
            self.filter_base = self.ctx.filter_get()
            self.ctx.filter_delta_reset()
            self.pfilter_base = ([self.ctx.policy_filter_get(p) for p in range(P)]
                                 if self.cfg.policy_filter else None)
            self.ctx.policy_filter_delta_reset()
            self.grad = torch.zeros(self.ctx.n_params[0], dtype=torch.float32, device=self.device)
        self.workers = _Workers(self)
        self.rctx.observe(self.backend.reset())

    # -- one iteration ---------------------------------------------------------------
    def _sample(self):
        self._sample_fragment()
        self._sample_finish()

    def _init_device_rng(self, noise_seed, sched_seed):
        """rng_backend "device": seed the two streams and allocate what they fill -- one noise slab
        [T, N, agents, A] of a whole fragment and the learner's persistent schedule arrays."""
        from .envs import DeviceVecEnv
        torch, cfg = self.torch, self.cfg
        self.rctx.rng_seed(N.RNG_NOISE, noise_seed)
        self.ctx.rng_seed(N.RNG_SCHEDULE, sched_seed)
        self.noise = torch.empty((self.T, self.n_envs, cfg.n_agents, cfg.act_dim), dtype=torch.float32,
                                 device=self.device)
        self.sched = self.ctx.schedule_alloc(self.device)
        # on the device env plane the fragment is one chain (ddrl_rollout_devenv); False runs the
        # per-step loop over the same slab (the same results; the other planes always do)
        self.fragment_chain = isinstance(self.backend, DeviceVecEnv)

    def _sample_fragment(self):
        """The fragment: T steps of act / env step / reward / observe, then the bootstrap.
        (A population replaces its members' loops by one group chain: ddrl_amd.population.)"""
        torch, cfg = self.torch, self.cfg
        rctx = self.rctx
        if self.rng_backend == "device":
            rctx.noise_fill(self.T, self.noise)
            if self.fragment_chain:   # the slab's address is fixed: the captured graph is replayed
                rctx.rollout_devenv(self.backend.env, self.noise)
                return
        for t in range(self.T):
            eps = self.noise[t] if self.rng_backend == "device" else torch.randn(
                (self.n_envs, cfg.n_agents, cfg.act_dim), device=self.device, generator=self.noise_gen)
            rctx.act(t, eps, self.actions)
            obs, fw, cfrc, done = self.backend.step(self.actions)
            rctx.reward(t, fw, cfrc, self.actions, done)
            rctx.observe(obs)
        rctx.bootstrap()

    def _sample_finish(self):
        """The part after the fragment (this trainer's own, or a group's): advantages, the episode
        accounting and the cross-rank syncs."""
        rctx = self.rctx
        rctx.gae()
        self._episode_rows = self._collect_episodes()
        if self.parallel == "gather":
            from .ddp import sync_filters, sync_standardize, standardize_constants
            for p in range(self.cfg.n_policies):
                if self.pfilter_base is not None:   # RLlib synchronize_filters
                    d = rctx.policy_filter_get(p, delta=True)
                    self.pfilter_base[p] = (sync_filters(self.comm, self.pfilter_base[p], d) if self.comm else
                                            sync_filters_local(self.pfilter_base[p], d))
                    rctx.policy_filter_set(p, *self.pfilter_base[p])
                    self.ctx.policy_filter_set(p, *self.pfilter_base[p])
                sums = rctx.adv_sums_get(p)
                norm = sync_standardize(self.comm, sums) if self.comm else standardize_constants(sums)
                self.ctx.adv_norm_set(p, *norm)
            rctx.policy_filter_delta_reset()
            return
        if self.parallel == "ddp":
            from .ddp import sync_filters, sync_standardize
            # The env-side MeanStdFilter is a per-process singleton in the reference
            # (simulation_envs/observation_filter.py:3-12) that RLlib never synchronizes: it stays
            # rank-local unless the config asks for a merged one ("sync_env_filter": True, an
            # extension).  RLlib's per-policy filters are synchronized (synchronize_filters).
            if self.config.get("sync_env_filter", False):
                merged = sync_filters(self.comm, self.filter_base, self.ctx.filter_delta_get())
                self.ctx.filter_set(*merged)
                self.ctx.filter_delta_reset()
                self.filter_base = merged
            if self.pfilter_base is not None:   # RLlib synchronize_filters for the policy filters
                for p in range(self.cfg.n_policies):
                    self.pfilter_base[p] = sync_filters(self.comm, self.pfilter_base[p],
                                                        self.ctx.policy_filter_get(p, delta=True))
                    self.ctx.policy_filter_set(p, *self.pfilter_base[p])
                self.ctx.policy_filter_delta_reset()
            for p in range(self.cfg.n_policies):
                self.ctx.adv_norm_set(p, *sync_standardize(self.comm, self.ctx.adv_sums_get(p)))

    def _collect_episodes(self):
        """The episodes that finished in this fragment, [n, 8] rows in (t, env) order.  Across
        ranks: counts and padded rows are all-gathered and merged with the global env index
        rank * n_envs + env, so every rank reports the numbers of one process over all envs."""
        rows = self.rctx.episodes_collect()
        comm = getattr(self, "comm", None)
        if self.world == 1 or comm is None:
            return rows
        return gather_rank_rows(comm, rows, self.n_envs)

    def _schedule(self, p):
        """SampleBatch.shuffle() + one permutation of the minibatch slots per epoch."""
        R = self.T * self.ctx.layout[p]["C"]
        mb = self.cfg.sgd_minibatch_size
        shuffle = self.sched_rng.permutation(R).astype(np.int32)
        nb = max(1, R // mb)
        perms = np.stack([self.sched_rng.permutation(nb) for _ in range(self.cfg.num_sgd_iter)]).astype(np.int32)
        return shuffle, perms, nb

    def _learn_ddp(self):
        torch = self.torch
        R = self.T * self.ctx.layout[0]["C"]
        shuffle, perms = self.learner.schedule(self.sched_rng, R, self.cfg.num_sgd_iter)
        kl = self.learner.learn(torch.from_numpy(shuffle).to(self.device), perms, self.kl_coeff[0], self.grad)
        nb = perms.shape[1]
        last = self.ctx.ppo_stats(0, nb, self.learner.stats_first).astype(np.float64).mean(0)
        pid = self.policy_ids[0]
        learner = {pid: {"cur_kl_coeff": float(np.float32(self.kl_coeff[0])),
                         "cur_lr": float(np.float32(self.cfg.lr)), "total_loss": last[0],
                         "policy_loss": last[1], "vf_loss": last[2], "kl": kl, "entropy": last[4],
                         "vf_explained_var": last[5], "entropy_coeff": self.cfg.entropy_coeff,
                         "num_ranks": self.world}}
        self.kl_coeff[0] = update_kl(self.kl_coeff[0], kl, self.config["kl_target"])
        return learner

    def _gather_records(self):
        """All-gather every rank's records (rank-major) into the learner context's union batch."""
        from .ddp import gather_records
        for p in range(self.cfg.n_policies):
            gather_records(self.comm, self.rctx.records_tensor(p), self.ctx.records_tensor(p))

    def _learn(self):
        if self.parallel == "ddp":
            return self._learn_ddp()
        if self.parallel == "gather":
            self._gather_records()
        sh, pe, nbs = self._learn_schedules()
        self.ctx.ppo_update((1 << self.cfg.n_policies) - 1, sh, pe, self.kl_coeff)
        return self._learn_results(nbs)

    def _learn_schedules(self, fill=True):
        """The part of the fused update before its launch: every policy's schedule on the device,
        drawn from this trainer's sched_rng in policy order.  (shuffles, perms, minibatches per epoch)
        rng_backend "device": one fill of the persistent arrays from the learner context's schedule
        stream (fill=False: a population has filled its members' arrays in one group launch)."""
        torch = self.torch
        if self.rng_backend == "device":
            if fill:
                self.ctx.schedule_fill(*self.sched)
            return self.sched[0], self.sched[1], [int(q.shape[1]) for q in self.sched[1]]
        sh, pe, nbs = [], [], []
        for p in range(self.cfg.n_policies):
            s, q, nb = self._schedule(p)
            sh.append(torch.from_numpy(s).to(self.device))
            pe.append(torch.from_numpy(q).to(self.device))
            nbs.append(nb)
        return sh, pe, nbs

    def _last_epoch_stats(self, nbs):
        """The last epoch's statistics rows of every policy, float32 [nbs[p], 8] each."""
        return [self.ctx.ppo_stats(p, nbs[p], first=(self.cfg.num_sgd_iter - 1) * nbs[p])
                for p in range(self.cfg.n_policies)]

    def _learn_results(self, nbs, stats=None):
        """The part after the launch (this trainer's own, or a group's: ddrl_amd.population): the last
        epoch's statistics, update_kl and the learner dict.  stats: the rows of _last_epoch_stats when
        the caller has read them already (a population reads all members' in one call)."""
        P = self.cfg.n_policies
        if stats is None:
            stats = self._last_epoch_stats(nbs)
        learner = {}
        for p, pid in enumerate(self.policy_ids):
            last = stats[p].astype(np.float64).mean(0)   # TrainTFMultiGPU: last epoch's mean
            learner[pid] = {"cur_kl_coeff": float(np.float32(self.kl_coeff[p])),
                            "cur_lr": float(np.float32(self.cfg.lr)),
                            "total_loss": last[0], "policy_loss": last[1], "vf_loss": last[2],
                            "kl": last[3], "entropy": last[4], "vf_explained_var": last[5],
                            "grad_gnorm": last[6], "entropy_coeff": self.cfg.entropy_coeff}
            self.kl_coeff[p] = update_kl(self.kl_coeff[p], last[3], self.config["kl_target"])
        if self.parallel == "gather":   # the next rollout uses the updated weights
            for p in range(P):
                self.rctx.params_set(p, self.ctx.params_get(p))
        return learner

    def train(self):
        torch = self.torch
        t0 = time.perf_counter()
        self._sample()
        torch.cuda.synchronize(self.device)
        t1 = time.perf_counter()
        learner = self._learn()
        return self._iteration_result(learner, t0, t1, time.perf_counter())

    def _iteration_result(self, learner, t0, t1, t2):
        """The end of an iteration: counters, callback and RLlib's result dict.  t0 / t1 / t2: start,
        end of sampling, end of learning."""
        steps = self.T * self.n_envs
        self.timesteps_total += steps
        self.iteration += 1
        cb = self.config.get("callbacks", {}).get("on_train_result") if isinstance(
            self.config.get("callbacks"), dict) else None
        self.last_learner = learner
        # RLlib's result: the episode summary first (summarize_episodes' key order), then the
        # trainer's own keys -- Tune's progress.csv columns 0-6 follow from this order
        result = self.episode_history.summarize(self._episode_rows, list(self.cfg.agent_policy)[:self.cfg.n_agents],
                                                self.policy_ids)
        self.episodes_total += result["episodes_this_iter"]
        result.update({"num_healthy_workers": self.world, "timesteps_total": self.timesteps_total,
                       "timers": {"sample_time_ms": (t1 - t0) * 1e3, "learn_time_ms": (t2 - t1) * 1e3,
                                  "sample_throughput": steps / (t1 - t0),
                                  "learn_throughput": steps / (t2 - t1)},
                       "info": {"learner": learner}, "done": False, "episodes_total": self.episodes_total,
                       "training_iteration": self.iteration, "timesteps_this_iter": steps})
        if cb:
            cb({"result": result, "trainer": self})
        return result

    # -- state -------------------------------------------------------------------------
    def get_weights(self):
        return {pid: self.ctx.params_get(p) for p, pid in enumerate(self.policy_ids)}

    def set_weights(self, weights):
        """Writes the learner context and, in "gather" mode, the rollout context too: the next
        fragment must be sampled (and its logp / vf recorded) with the weights it trains."""
        for p, pid in enumerate(self.policy_ids):
            if pid in weights:
                self.ctx.params_set(p, weights[pid])
                if self.rctx is not self.ctx:
                    self.rctx.params_set(p, weights[pid])

    def save(self, path):
        """Checkpoint: weights, Adam m/v/beta powers, KL coefficients, filter state and, with
        rng_backend "device", the state of the noise and schedule streams (npz, no pickle)."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        arrs = {}
        for p, pid in enumerate(self.policy_ids):
            m, v, b1, b2 = self.ctx.adam_get(p)
            arrs[f"{pid}/weights"] = self.ctx.params_get(p)
            arrs[f"{pid}/adam_m"], arrs[f"{pid}/adam_v"] = m, v
            arrs[f"{pid}/beta_powers"] = np.array([b1, b2], np.float32)
            arrs[f"{pid}/kl_coeff"] = np.array([self.kl_coeff[p]])
        n, M, S = self.rctx.filter_get()   # the env-side filter lives where the rollout runs
        arrs["filter/n"], arrs["filter/M"], arrs["filter/S"] = np.array([n]), M, S
        if self.cfg.policy_filter:
            for p, pid in enumerate(self.policy_ids):
                n, M, S = self.ctx.policy_filter_get(p)
                arrs[f"{pid}/filter/n"], arrs[f"{pid}/filter/M"], arrs[f"{pid}/filter/S"] = np.array([n]), M, S
        meta = {"iteration": self.iteration, "timesteps_total": self.timesteps_total}
        if self.rng_backend == "device":   # (seed, position) of both streams: all of the generator's state
            meta["rng"] = {"noise": list(self.rctx.rng_state(N.RNG_NOISE)),
                           "schedule": list(self.ctx.rng_state(N.RNG_SCHEDULE))}
        arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
        np.savez(path, **arrs)
        return path

    def restore(self, path):
        z = np.load(path, allow_pickle=False)
        for p, pid in enumerate(self.policy_ids):
            self.ctx.params_set(p, z[f"{pid}/weights"])
            if self.rctx is not self.ctx:
                self.rctx.params_set(p, z[f"{pid}/weights"])
            b = z[f"{pid}/beta_powers"]
            self.ctx.adam_set(p, z[f"{pid}/adam_m"], z[f"{pid}/adam_v"], float(b[0]), float(b[1]))
            self.kl_coeff[p] = float(z[f"{pid}/kl_coeff"][0])
        self.rctx.filter_set(float(z["filter/n"][0]), z["filter/M"], z["filter/S"])
        if self.cfg.policy_filter:
            for p, pid in enumerate(self.policy_ids):
                for cx in {id(self.ctx): self.ctx, id(self.rctx): self.rctx}.values():
                    cx.policy_filter_set(p, float(z[f"{pid}/filter/n"][0]), z[f"{pid}/filter/M"],
                                         z[f"{pid}/filter/S"])
        meta = json.loads(bytes(z["meta"]).decode())
        self.iteration, self.timesteps_total = meta["iteration"], meta["timesteps_total"]
        if self.rng_backend == "device" and "rng" in meta:   # files without the streams keep the trainer's own
            self.rctx.rng_state_set(N.RNG_NOISE, *meta["rng"]["noise"])
            self.ctx.rng_state_set(N.RNG_SCHEDULE, *meta["rng"]["schedule"])
        self._after_load({})

    def _after_load(self, learner):
        """State that follows a restore: the learner statistics that belong to the restored
        weights (none for an npz checkpoint, the file's own for an RLlib one), and, for the
        data-parallel / gather modes, the base of the per-policy filter sync, which must be the
        restored RunningStat (else the next sync merges the delta into the stale base)."""
        self.last_learner = learner
        if self.parallel in ("ddp", "gather") and getattr(self, "pfilter_base", None) is not None:
            self.pfilter_base = [self.ctx.policy_filter_get(p) for p in range(self.cfg.n_policies)]
            self.rctx.policy_filter_delta_reset()

    def restore_rllib(self, path):
        """Load a published RLlib checkpoint (Results/**/checkpoint-1250, the file
        evaluation/evaluate_trained_policies_pd.py:93-96 restores): per policy the Keras-order
        weights, Adam m / v and beta powers, the RLlib MeanStdFilter RunningStat (when this
        trainer runs observation_filter = MeanStdFilter) and the KL coefficient.  Read with the
        no-code reader (ddrl_amd.rllib_checkpoint: a pickletools opcode walk; nothing in the
        file is executed).  Returns the policy ids loaded."""
        from .rllib_checkpoint import policy_ids, policy_state, read_checkpoint
        ck = read_checkpoint(path)
        return self.load_policy_states({pid: policy_state(ck, pid) for pid in policy_ids(ck)})

    def rllib_policy_states(self):
        """Per policy id the state rllib_checkpoint.worker_tree writes: Keras-order weights,
        Adam m / v, beta powers, the RLlib MeanStdFilter RunningStat (when this trainer runs
        observation_filter = MeanStdFilter; NoFilter otherwise) and the variable shapes."""
        from .rllib_checkpoint import ffn_shapes, gnn_shapes
        out = {}
        A = self.cfg.act_dim
        for p, pid in enumerate(self.policy_ids):
            m, v, b1, b2 = self.ctx.adam_get(p)
            d = int(self.cfg.obs_dim[p])
            if self.cfg.model_kind == N.MODEL_FFN:
                shapes = ffn_shapes(d, 2 * A) + ([("leg_coupling", (4, A))] if self.cfg.leg_coupling else [])
            else:
                shapes = gnn_shapes(2 * A, layer={v: k for k, v in N.GNN_LAYERS.items()}[self.cfg.gnn_layer])
            st = {"weights": self.ctx.params_get(p), "adam_m": m, "adam_v": v,
                  "beta_powers": (np.float32(b1), np.float32(b2)), "shapes": shapes, "obs_dim": d,
                  "filter": None, "filter_buffer": None}
            if self.cfg.policy_filter:
                st["filter"] = self.ctx.policy_filter_get(p)
            else:
                st["filter_kind"] = "NoFilter"
            out[pid] = st
        return {pid: out[pid] for pid in sorted(out)}   # Ray 1.0.1 writes the policies sorted by id

    def save_rllib(self, checkpoint_dir, time_total=0.0, episodes_total=0):
        """Write an RLlib (Ray 1.0.1) checkpoint of this trainer --
        <checkpoint_dir>/checkpoint_<i>/checkpoint-<i> + .tune_metadata -- in the layout
        PPOTrainer.restore reads (evaluation/evaluate_trained_policies_pd.py:93-96), with the
        learner statistics of the last train() call.  The writer emits the pickle opcodes
        itself (ddrl_amd.rllib_checkpoint.emit); it reproduces every published checkpoint
        byte for byte from its contents (tests/test_checkpoint.py)."""
        from .rllib_checkpoint import write_checkpoint
        last = getattr(self, "last_learner", {}) or {}
        learner = {}
        for p, pid in enumerate(self.policy_ids):
            s = dict(last.get(pid, {}))
            # no statistics for the current weights (no train() since the trainer was built or
            # restored from an npz file): the row carries the current coefficient and no "kl",
            # so a reload keeps the coefficient as it is (load_policy_states runs update_kl only
            # with a kl)
            s.setdefault("cur_kl_coeff", float(np.float32(self.kl_coeff[p])))
            s.setdefault("cur_lr", float(np.float32(self.cfg.lr)))
            s.setdefault("entropy_coeff", float(self.cfg.entropy_coeff))
            learner[pid] = s
        return write_checkpoint(checkpoint_dir, self.iteration, self.rllib_policy_states(), learner,
                                self.timesteps_total, time_total=time_total, episodes_total=episodes_total)

    def load_policy_states(self, states):
        """Per policy id: {"weights", "adam_m", "adam_v", "beta_powers", "filter" (n, M, S) or
        None, "kl_coeff" or None} (ddrl_amd.rllib_checkpoint.policy_state's layout) into the
        context; returns the policy ids loaded."""
        missing = [pid for pid in self.policy_ids if pid not in states]
        learner = {}
        if missing:
            raise ValueError(f"checkpoint has policies {sorted(states)}, this env needs {self.policy_ids}")
        for p, pid in enumerate(self.policy_ids):
            st = states[pid]
            if st["weights"].size != self.ctx.n_params[p]:
                raise ValueError(f"{pid}: checkpoint holds {st['weights'].size} parameters, the model "
                                 f"{self.ctx.n_params[p]}")
            self.ctx.params_set(p, st["weights"])
            self.ctx.adam_set(p, st["adam_m"], st["adam_v"], *st["beta_powers"])
            if self.cfg.policy_filter and st["filter"] is not None:
                self.ctx.policy_filter_set(p, *st["filter"])
                self.rctx.policy_filter_set(p, *st["filter"])
            if self.rctx is not self.ctx:
                self.rctx.params_set(p, st["weights"])
            stats = dict(st.get("learner_stats") or {})
            if self.config.get("restore_kl_coeff", "checkpoint") == "config":
                # RLlib 1.0.1: the TF policy state holds only model and optimizer variables
                # (KLCoeffMixin has no get_state), so PPOTrainer.restore starts again from
                # config["kl_coeff"]
                self.kl_coeff[p] = float(self.config["kl_coeff"])
                stats.pop("kl", None)
                stats["cur_kl_coeff"] = self.kl_coeff[p]
            elif st["kl_coeff"] is not None:
                # extension: continue from the file's coefficient.  Its
                # cur_kl_coeff is the coefficient the checkpointed iteration trained with; the
                # next iteration's is update_kl of it and that iteration's kl (RLlib runs update_kl
                # after the learner step, ppo.py UpdateKL)
                kl = stats.get("kl")
                self.kl_coeff[p] = (update_kl(st["kl_coeff"], kl, self.config["kl_target"]) if kl is not None
                                    else st["kl_coeff"])
                stats["cur_kl_coeff"] = st["kl_coeff"]
            learner[pid] = stats
        self._after_load(learner)
        return list(self.policy_ids)

    # -- evaluation ----------------------------------------------------------------------
    def _eval_context(self, n_envs, env_config=None):
        """A separate context of n_envs envs (cached per shape) holding a copy of the current
        weights and per-policy filters; the training context is only read."""
        cache = self.__dict__.setdefault("_eval_ctx", {})
        key = (int(n_envs), json.dumps(env_config, sort_keys=True))
        if key not in cache:
            config = self.config if env_config is None else {
                **self.config, "env_config": {**self.config.get("env_config", {}), **env_config}}
            cfg, _ = make_cfg(self.config["env"], n_envs, 1, config)
            cache[key] = N.Context(cfg, self.device.index, self.stream.cuda_stream)
        ectx = cache[key]
        for p in range(self.cfg.n_policies):
            ectx.params_set(p, self.ctx.params_get(p))
            if self.cfg.policy_filter:
                ectx.policy_filter_set(p, *self.ctx.policy_filter_get(p))
        return ectx

    def evaluate(self, num_episodes=100, num_steps=1000, explore=True, tvel=None, n_envs=None,
                 env_filter="continue", seed=0, env_backend="host", hf_smoothness=None):
        """Run the current policies for whole episodes over the host env plane and return the
        reference's tuple (reward_eps, steps_eps, dist_eps, power_total_eps, vel_eps, cot_eps) of
        evaluation/rollout_episodes.py:26-164, one entry per episode.

        n_envs (default min(num_episodes, 128)) envs run E = ceil(num_episodes / n_envs) episodes
        each, side by side, instead of the reference's sequential episodes; the result is the first
        num_episodes completed rows in env-major order.  A fixed quota per env keeps short episodes
        from being over-represented.  num_steps is the episode length limit (:83).

        explore=True is the default because the reference calls compute_action without `explore`
        (:103-107), so RLlib samples from the action distribution; explore=False takes the mean.
        tvel: a one-entry target-velocity list (:38-39).  env_filter: the env-side MeanStdFilter
        of the evaluation -- "continue": a copy of the training filter that keeps updating (the
        reference's singleton does, quantruped_adaptor_multi_environment.py:83-85), "frozen": the
        copy, not updated, "fresh": a new filter, updating (what the reference's separate
        evaluation process gets).  The per-policy filters are applied without updates, as RLlib's
        compute_action does.  The training context, its env backend and the noise generator are
        not touched: evaluation runs on its own context, env plane and generator (`seed`).

        env_backend: "host" (the default) steps the envs on host threads; "device" steps them in
        a kernel on the evaluation context's stream (ddrl_eval_devenv: no copies, one
        synchronization per progress poll), and n_envs then defaults to min(num_episodes, 4096).

        hf_smoothness: the smoothness of the ground the evaluation env plane is created with (1.0:
        flat); None takes the trainer's env_config["hf_smoothness"].  Every episode of every env
        runs on ground of its own (the field is keyed by the env's episode number), as the reference
        makes a new field before every episode (evaluation/rollout_episodes.py:79)."""
        return self._evaluate(num_episodes, num_steps, explore, tvel, n_envs, env_filter, seed,
                              env_backend=env_backend, hf_smoothness=hf_smoothness)[0]

    def _evaluate(self, num_episodes, num_steps, explore, tvel, n_envs, env_filter, seed, sens_steps=None,
                  env_backend="host", hf_smoothness=None):
        """The body of evaluate / evaluate_sensitivity: (six lists, per-policy sensitivity results or
        None).  sens_steps: a function of the evaluation context returning the per-policy steps;
        with it, the C++ loop runs the sensitivity kernel after every action."""
        if env_filter not in ("continue", "frozen", "fresh"):
            raise ValueError(f"env_filter {env_filter!r}: 'continue', 'frozen' or 'fresh'")
        if env_backend not in ("host", "device"):
            raise ValueError(f"env_backend {env_backend!r}: 'host' or 'device'")
        if self.cfg.model_kind != N.MODEL_FFN:
            raise N.DdrlError("evaluation: fcnet models only")
        torch, cfg = self.torch, self.cfg
        num_episodes, num_steps = int(num_episodes), int(num_steps)
        if num_episodes < 1 or num_steps < 1:
            raise ValueError("num_episodes and num_steps must be >= 1")
        n_envs = int(n_envs or min(num_episodes, 4096 if env_backend == "device" else 128))
        E = -(-num_episodes // n_envs)
        ectx = self._eval_context(n_envs)
        D = cfg.obs_full_dim
        if env_filter == "fresh":
            ectx.filter_set(0.0, np.zeros(D), np.zeros(D))
        else:
            ectx.filter_set(*self.rctx.filter_get())
        tv = [float(tvel)] if tvel else [float(v) for v in (self.env.target_velocity_list or [0.0])]
        if env_backend == "device":
            henv = N.DevEnv(ectx, seed=seed, target_velocity=tv if len(tv) > 1 else tv[0])
        else:
            henv = N.HostEnv(n_envs, D, n_threads=int(self.config.get("num_host_threads", 4)), seed=seed,
                             target_velocity=tv if len(tv) > 1 else tv[0])
        run = ectx.eval_devenv if env_backend == "device" else ectx.eval_hostenv
        try:
            henv.set_time_limit(num_steps)
            henv.set_terrain(self.hf_smoothness if hf_smoothness is None else float(hf_smoothness))
            max_steps = E * num_steps   # every env has had E episodes by then
            eps = None
            if explore:
                gen = torch.Generator(device=self.device)
                gen.manual_seed(seed + 1)
                eps = torch.randn((max_steps, n_envs, cfg.n_agents, cfg.act_dim), device=self.device, generator=gen)
            ectx.eval_begin(E, filter_update=env_filter != "frozen")
            if sens_steps is not None:
                ectx.eval_sens_begin(sens_steps(ectx))
            run(henv, eps, max_steps if explore else 0, max_steps, poll_every=min(25, num_steps))
            rows = ectx.eval_results().reshape(-1, 6)
            sens = None
            if sens_steps is not None:
                sens = {}
                for p, pid in enumerate(self.policy_ids):
                    g, ga, n = ectx.eval_sens_results(p)
                    sens[pid] = {"grads": g, "grads_abs": ga, "rows": n}
            ectx.eval_end()
        finally:
            henv.close()
        rows = rows[~np.isnan(rows[:, 1])][:num_episodes]
        reward, steps, dist, power, vel, cot = (rows[:, i].tolist() for i in range(6))
        return (reward, [int(s) for s in steps], dist, power, vel, cot), sens

    def evaluate_members(self, members, num_episodes=10, num_steps=1000, explore=True, env_filter="continue", seed=0,
                         hf_smoothness=None):
        """evaluate() of many parameter sets side by side, the cells of the reference's sweeps
        (evaluation/evaluate_trained_policies_pd.py:84-127, one restored agent per seed;
        evaluate_trained_policies_tvel_range_pd.py:80-102, one per seed and target velocity) as one
        evaluation.  members: a list of (checkpoint_path or None, tvel or None) -- None: the
        trainer's current state, its configured velocity.  Returns one six-list tuple per member.

        Always on the device env plane, on the trainer's evaluation context of M * n envs with the
        member mode on (ddrl_eval_members_begin): n = min(num_episodes, 4096 // M) envs per member,
        E = ceil(num_episodes / n) episodes per env, member m on the envs [m n, (m + 1) n).  Every
        member has its own weights, per-policy filters and env-side filter (env_filter as in
        evaluate(), applied per member: each starts from the training filter, or fresh, and keeps
        its own statistics).  A checkpoint (an RLlib checkpoint file, read with the no-code reader)
        is written into the evaluation context only: the training and rollout contexts, their Adam
        state and filters are not touched.  Members whose tvel is None on a trainer with several
        configured velocities draw from that list, as evaluate() does."""
        members = [tuple(m) for m in members]
        M = len(members)
        if M < 1:
            raise ValueError("evaluate_members: at least one member")
        if M > 4096:
            raise ValueError(f"evaluate_members: {M} members, at most 4096 (one env each) fit an evaluation; "
                             "split the sweep (ddrl_amd.evaluation.evaluate_sweep does)")
        if any(len(m) != 2 for m in members):
            raise ValueError("evaluate_members: members are (checkpoint_path or None, tvel or None) pairs")
        for _, tvel in members:
            if tvel is not None and not (np.isfinite(float(tvel)) and float(tvel) > 0.0):
                raise ValueError(f"evaluate_members: target velocity {tvel!r} must be finite and > 0")
        if env_filter not in ("continue", "frozen", "fresh"):
            raise ValueError(f"env_filter {env_filter!r}: 'continue', 'frozen' or 'fresh'")
        num_episodes, num_steps = int(num_episodes), int(num_steps)
        if num_episodes < 1 or num_steps < 1:
            raise ValueError("num_episodes and num_steps must be >= 1")
        if self.cfg.model_kind != N.MODEL_FFN:
            raise N.DdrlError("evaluation: fcnet models only")
        from .rllib_checkpoint import policy_ids, policy_state, read_checkpoint
        torch, cfg = self.torch, self.cfg
        n = min(num_episodes, 4096 // M)
        E = -(-num_episodes // n)
        n_envs = M * n
        # the checkpoints, read and checked before anything is launched
        states = {}
        for path, _ in members:
            if path is None or path in states:
                continue
            ck = read_checkpoint(path)
            st = {pid: policy_state(ck, pid) for pid in policy_ids(ck)}
            missing = [pid for pid in self.policy_ids if pid not in st]
            if missing:
                raise ValueError(f"{path}: checkpoint has policies {sorted(st)}, this env needs {self.policy_ids}")
            for p, pid in enumerate(self.policy_ids):
                if st[pid]["weights"].size != self.ctx.n_params[p]:
                    raise ValueError(f"{path}: {pid} holds {st[pid]['weights'].size} parameters, the model "
                                     f"{self.ctx.n_params[p]}")
            states[path] = st
        configured = [float(v) for v in (self.env.target_velocity_list or [0.0])]
        table = None
        if any(tvel is not None for _, tvel in members):
            if len(configured) > 1 and any(tvel is None for _, tvel in members):
                raise ValueError("evaluate_members: give every member a tvel, or none (the trainer draws from "
                                 f"{len(configured)} configured velocities)")
            table = np.repeat([configured[0] if tvel is None else float(tvel) for _, tvel in members], n)
        ectx = self._eval_context(n_envs)   # holds the trainer's current weights and per-policy filters
        D = cfg.obs_full_dim
        if env_filter == "fresh":
            ectx.filter_set(0.0, np.zeros(D), np.zeros(D))
        else:
            ectx.filter_set(*self.rctx.filter_get())
        current = None   # the trainer's own state, once a checkpoint has overwritten the context's copy
        henv = N.DevEnv(ectx, seed=seed, target_velocity=configured if len(configured) > 1 else configured[0])
        try:
            henv.set_time_limit(num_steps)
            henv.set_terrain(self.hf_smoothness if hf_smoothness is None else float(hf_smoothness))
            if table is not None:
                henv.set_env_target_velocities(table)
            max_steps = E * num_steps
            eps = None
            if explore:
                gen = torch.Generator(device=self.device)
                gen.manual_seed(seed + 1)
                eps = torch.randn((max_steps, n_envs, cfg.n_agents, cfg.act_dim), device=self.device, generator=gen)
            ectx.eval_begin(E, filter_update=env_filter != "frozen")
            ectx.eval_members_begin(M)
            for m, (path, _) in enumerate(members):
                if path is not None and current is None:
                    current = [(ectx.params_get(p), ectx.policy_filter_get(p) if cfg.policy_filter else None)
                               for p in range(cfg.n_policies)]
                for p, pid in enumerate(self.policy_ids):
                    if path is not None:
                        st = states[path][pid]
                        ectx.params_set(p, st["weights"])
                        if cfg.policy_filter:
                            ectx.policy_filter_set(p, *(st["filter"] if st["filter"] is not None else current[p][1]))
                    elif current is not None:
                        ectx.params_set(p, current[p][0])
                        if cfg.policy_filter:
                            ectx.policy_filter_set(p, *current[p][1])
                ectx.eval_member_load(m)
            ectx.eval_devenv(henv, eps, max_steps if explore else 0, max_steps, poll_every=min(25, num_steps))
            rows = ectx.eval_results().reshape(M, n * E, 6)
            ectx.eval_end()
        finally:
            henv.close()
        out = []
        for m in range(M):
            r = rows[m]
            r = r[~np.isnan(r[:, 1])][:num_episodes]
            reward, steps, dist, power, vel, cot = (r[:, i].tolist() for i in range(6))
            out.append((reward, [int(s) for s in steps], dist, power, vel, cot))
        return out

    def evaluate_sensitivity(self, num_episodes=10, num_steps=1000, rel_step=0.1, steps=None, tvel=None, n_envs=None,
                             env_filter="continue", seed=0, explore=True, env_backend="host", hf_smoothness=None):
        """evaluate() plus the importance matrix of the reference's
        evaluation/rollout_episodes_compute_gradient.py:59-68, :111-122: at every control step every
        input of every policy row is moved by -h_f / +h_f and the difference of the clipped action
        means (explore=False) is summed into grads[f][j], its magnitude into grads_abs[f][j] (fp64),
        over the steps of exactly the episodes of the result lists (an env stops contributing when
        its quota is full).  Returns (six lists, {policy_id: {"grads": [d, A], "grads_abs": [d, A],
        "rows": int}}); the six lists are evaluate()'s for the same arguments.

        Steps: with the per-policy filter (observation_filter: MeanStdFilter) h_f = rel_step * std_f,
        std_f = sqrt(S_f / (n - 1)) of that filter, as the reference's 0.1 * rs.std.  Without it
        (an extension: the reference only runs the filtered centralized policy) h_f = rel_step * 1.0,
        the env-normalized columns having unit scale.  `steps` ({policy_id: [d]} or a per-policy
        list) overrides both.  Every policy of every architecture gets a matrix; constant inputs
        (the LegID one-hot) are not moved and their rows stay zero.  env_backend and hf_smoothness as in evaluate()."""
        from .evaluation import default_sens_steps

        def sens_steps(ectx):
            out = []
            for p, pid in enumerate(self.policy_ids):
                d = int(self.cfg.obs_dim[p])
                given = None if steps is None else (steps.get(pid) if isinstance(steps, dict) else steps[p])
                if given is not None:
                    h = np.asarray(given, np.float64).reshape(-1)
                    if h.size != d:
                        raise ValueError(f"steps for {pid!r}: {h.size} values, the policy takes {d}")
                elif self.cfg.policy_filter:
                    n, M, S = ectx.policy_filter_get(p)
                    h = default_sens_steps(n, S, rel_step, M)
                else:
                    h = np.full(d, float(rel_step))
                out.append(h)
            return out

        return self._evaluate(num_episodes, num_steps, explore, tvel, n_envs, env_filter, seed, sens_steps,
                              env_backend=env_backend, hf_smoothness=hf_smoothness)

    def compute_action(self, obs, policy_id=None, explore=None, seed=None, agent_id=None):
        """Trainer.compute_action for one agent observation (the policy's input row, as the env
        adaptor hands it out): the per-policy filter without update, the policy forward and the
        action, clipped to [-1, 1] (clip_actions).  explore None / True samples (RLlib's default),
        False takes the mean.  Runs through ddrl_eval_act on a one-env context whose env-side
        filter is off, with the row placed at the agent's columns of a full observation.
        agent_id (default: the policy's first agent) selects the leg row of the "cup" model."""
        policy_id = self.policy_ids[0] if policy_id is None else policy_id
        p = self.policy_ids.index(policy_id)
        cfg, torch = self.cfg, self.torch
        A, d = cfg.act_dim, int(cfg.obs_dim[p])
        obs = np.asarray(obs, np.float32).reshape(-1)
        if obs.size != d:
            raise ValueError(f"{policy_id}: observation of {obs.size} values, the policy takes {d}")
        ectx = self._eval_context(1, {"observation_filter_env": False})
        agents = [j for j in range(cfg.n_agents) if cfg.agent_policy[j] == p]
        j = agents[0] if agent_id is None else list(self.env.agent_names).index(agent_id)
        if j not in agents:
            raise ValueError(f"agent {agent_id!r} is not mapped to policy {policy_id!r}")
        full = np.zeros((1, cfg.obs_full_dim), np.float32)
        for f in range(d):
            i = ectx.cfg.obs_index[j][f]
            if i >= 0:
                full[0, i] = obs[f]
        dev = lambda a: torch.from_numpy(a).to(self.device)
        logits = [torch.zeros((len([a for a in range(cfg.n_agents) if cfg.agent_policy[a] == q]), 2 * A),
                              dtype=torch.float32, device=self.device) for q in range(cfg.n_policies)]
        actions = torch.zeros((1, 8), dtype=torch.float32, device=self.device)
        ectx.eval_begin(1)
        ectx.eval_act(dev(full), None, actions, logits)
        ectx.synchronize()
        ectx.eval_end()
        lg = logits[p][agents.index(j)].cpu().numpy()
        act = lg[:A].copy()
        if explore is None or explore:
            rng = np.random.default_rng(seed)
            act = act + np.exp(lg[A:]) * rng.standard_normal(A).astype(np.float32)
        return np.clip(act, -1.0, 1.0).astype(np.float32)

    def stop(self):
        for ectx in self.__dict__.pop("_eval_ctx", {}).values():
            ectx.close()
        if hasattr(self.backend, "close"):   # first: a device env plane is destroyed before its context
            self.backend.close()
        if self.rctx is not self.ctx:
            self.rctx.close()
        self.ctx.close()


class _EnvHandle:
    """What `worker.foreach_env(fn)` hands to fn: the env spec (the reference's MultiAgentEnv
    class surface), whose update_environment_after_epoch also resets the vectorized backend's
    envs (quantruped_adaptor_multi_environment.py:97-122: update_after_epoch, then env.reset())."""

    def __init__(self, trainer):
        self._trainer = trainer

    def update_environment_after_epoch(self, timesteps_total):
        self._trainer.env.update_environment_after_epoch(timesteps_total)
        hook = getattr(self._trainer.backend, "update_environment_after_epoch", None)
        if hook is not None:
            hook(timesteps_total)

    def __getattr__(self, name):
        return getattr(self._trainer.env, name)


class _Worker:
    def __init__(self, trainer):
        self._trainer = trainer

    def foreach_env(self, fn):
        """RolloutWorker.foreach_env: fn over this worker's envs -- one vectorized env here."""
        return [fn(_EnvHandle(self._trainer))]


class _Workers:
    """trainer.workers (RLlib WorkerSet) for the callbacks the reference's training scripts
    install: train_experiment_1_architecture_on_flat.py:171-178 runs
    trainer.workers.foreach_worker(lambda ev: ev.foreach_env(lambda env:
    env.update_environment_after_epoch(timesteps))) after every iteration."""

    def __init__(self, trainer):
        self._trainer = trainer

    def foreach_worker(self, fn):
        return [fn(_Worker(self._trainer))]


def sync_filters_local(base, delta):
    from .ddp import merge_running_stats
    return merge_running_stats(base, [delta])


def update_kl(kl_coeff, sampled_kl, kl_target=0.01):
    """RLlib PPO update_kl (ppo_tf_policy.KLCoeffMixin)."""
    if sampled_kl > 2.0 * kl_target:
        return kl_coeff * 1.5
    if sampled_kl < 0.5 * kl_target:
        return kl_coeff * 0.5
    return kl_coeff


def run(config, stop=None, n_envs=None, device=0, verbose=True, logdir=None):
    """tune.run("PPO", config=config, stop={"timesteps_total": ...}) for one trial.  stop may name
    any key of the result, e.g. {"episode_reward_mean": 500} (a nan mean -- no episode yet --
    never stops).  logdir: write Tune's progress.csv and result.json there (ProgressLogger)."""
    stop = stop or {"training_iteration": 1}
    tr = PPOTrainer(config, n_envs=n_envs, device=device)
    log = ProgressLogger(logdir) if logdir is not None else None
    results = []
    try:
        while True:
            r = tr.train()
            results.append(r)
            if log:
                log.on_result(r)
            if verbose:
                print(json.dumps({k: r[k] for k in ("training_iteration", "timesteps_total", "timers")}))
            if any(r.get(k, 0) >= v for k, v in stop.items()):
                break
    finally:
        if log:
            log.close()
    tr.stop()
    return results
