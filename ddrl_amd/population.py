"""Train several seeds of one experiment side by side.

A single run's fused PPO update is four sequential chains on 16 of the device's CUs, and it is
nearly the whole cost of an iteration.  The seeds of one experiment are independent runs of the
same shape, so their updates fit one launch (native.UpdateGroup, csrc/ppo_ffn_group.hip): member
m of a PopulationTrainer is, bit for bit, the solo PPOTrainer(config, seed=seeds[m]) -- its own
context, envs, noise, schedule, filters, KL coefficients and results -- with the M update launches
of an iteration replaced by one.  On the device env plane the members' fragments are one chain of
launches too (native.RolloutGroup, csrc/rollout_group.hip), each member drawing its noise from its
own generator as the solo trainer does.  On the synthetic and host planes sampling stays per member,
in stream order.  What follows a fragment -- GAE and the episode accounting -- is one chain for all
members on every plane (native.FinishGroup, csrc/finish_group.hip: it reads the records only), with
one host synchronize per population, and the learner statistics of an iteration are read in one call
(UpdateGroup.stats_range).  With rng_backend "device"
every member's generator is its context's pair of device streams, and the members' noise slabs
and schedules are one group launch each (native.noise_fill_group, native.schedule_fill_group)
instead of host draws member by member.
"""
from __future__ import annotations

import os
import time

from . import native as N
from .trainer import PPOTrainer


class PopulationTrainer:
    """M PPOTrainers on one device and stream, updated by one group launch per iteration.

    max_chains_per_launch: 0 = as many chains (members x policies) per launch as the device holds
    resident; a smaller value splits the update into several launches of whole members (the same
    results).  fcnet models, sgd_minibatch_size 128 and single-process replicas only: anything the
    group update refuses raises here, with its reason.
    group_rollout: None = the members' fragments as one group chain when every member runs the device
    env plane (env_backend "device"), member by member otherwise; True = the group chain, or an error
    with the reason; False = member by member.  The results are the same bit for bit.
    group_finish: None / True = GAE and the episode accounting of all members as one group chain, on
    every env plane; False = member by member.  The results are the same bit for bit.
    """

    def __init__(self, config, seeds, n_envs=None, device=0, max_chains_per_launch=0, group_rollout=None,
                 group_finish=None):
        import torch
        self.torch = torch
        self.seeds = [int(s) for s in seeds]
        torch.cuda.set_device(device)
        self.device = torch.device("cuda", device)
        self.stream = torch.cuda.current_stream(self.device)
        self.trainers = []
        self.group = None
        self.rollout_group = None
        self.finish_group = None
        try:
            for s in self.seeds:
                self.trainers.append(PPOTrainer(config, n_envs=n_envs, device=device, seed=s, stream=self.stream))
            for t in self.trainers:
                if t.world != 1 or t.parallel != "replicas":
                    raise ValueError(f"PopulationTrainer: parallel {t.parallel!r} over {t.world} process(es); a "
                                     "population is single-process replicas")
            # rng_backend "device" (one config: all members or none): group fills replace the host draws
            self.device_rng = bool(self.trainers) and self.trainers[0].rng_backend == "device"
            self.group = N.UpdateGroup([t.ctx for t in self.trainers], max_chains_per_launch)
            self._init_group_rollout(group_rollout)
            if group_finish is None or group_finish:
                self.finish_group = N.FinishGroup([t.rctx for t in self.trainers])
        except Exception:
            self.stop()
            raise

    def _init_group_rollout(self, group_rollout):
        """group_rollout None: the group rollout when every member runs the device env plane, the
        member-by-member sampling otherwise; True: the group rollout or an error with the reason;
        False: member by member."""
        from .envs import DeviceVecEnv
        on_device = bool(self.trainers) and all(isinstance(t.backend, DeviceVecEnv) for t in self.trainers)
        if group_rollout is None:
            group_rollout = on_device
        if not group_rollout:
            return
        if not on_device:
            raise ValueError("PopulationTrainer: group_rollout needs every member on the device env plane "
                             "(env_backend: 'device'); the synthetic and host planes sample member by member")
        self.rollout_group = N.RolloutGroup([t.rctx for t in self.trainers], [t.backend.env for t in self.trainers])
        # every member's noise of a fragment, [T, n_envs, n_agents, A], read by the group chain: filled
        # step by step from the member's own generator (the solo trainer's draw sequence), or, with
        # rng_backend "device", the members' own slabs filled by one group launch
        if self.device_rng:
            self.noise = [t.noise for t in self.trainers]
        else:
            self.noise = [self.torch.empty((t.T, t.n_envs, t.cfg.n_agents, t.cfg.act_dim), dtype=self.torch.float32,
                                           device=self.device) for t in self.trainers]

    def _sample_group(self):
        torch = self.torch
        if self.device_rng:
            N.noise_fill_group([t.rctx for t in self.trainers], self.trainers[0].T, self.noise)
        else:
            for t, slab in zip(self.trainers, self.noise):
                for step in range(t.T):
                    torch.randn(tuple(slab.shape[1:]), generator=t.noise_gen, out=slab[step])
        self.rollout_group.run(self.noise)

    def _finish(self):
        """What follows the members' fragments: one group chain, or every member's own calls."""
        if self.finish_group is None:
            for t in self.trainers:
                t._sample_finish()
            return
        # (a population's members are single-process replicas: _sample_finish has no cross-rank part)
        for t, rows in zip(self.trainers, self.finish_group.run()):
            t._episode_rows = rows

    def _learn_stats(self, nbs):
        """Every member's last-epoch statistics rows ([M] lists of [P] arrays) in one readback, or None
        where the policies' schedules differ in length (the members then read their own)."""
        if len(set(nbs)) != 1:
            return None
        a = self.group.stats_range((self.trainers[0].cfg.num_sgd_iter - 1) * nbs[0], nbs[0])
        return [list(a[m]) for m in range(len(self.trainers))]

    def train(self):
        """One iteration of every member; the list of the members' result dicts."""
        t0 = time.perf_counter()
        if self.rollout_group is not None:
            self._sample_group()
        else:
            for t in self.trainers:
                t._sample_fragment()
        self._finish()
        self.torch.cuda.synchronize(self.device)
        t1 = time.perf_counter()
        if self.device_rng:   # every member's schedule in one launch, into its own persistent arrays
            N.schedule_fill_group([t.ctx for t in self.trainers], [t.sched[0] for t in self.trainers],
                                  [t.sched[1] for t in self.trainers])
        sched = [t._learn_schedules(fill=False) for t in self.trainers]
        self.group.run([s[0] for s in sched], [s[1] for s in sched], [t.kl_coeff for t in self.trainers])
        self.group.finish()
        stats = self._learn_stats(sched[0][2]) if sched else None
        learners = [t._learn_results(s[2], stats[m] if stats else None)
                    for m, (t, s) in enumerate(zip(self.trainers, sched))]
        t2 = time.perf_counter()
        return [t._iteration_result(lr, t0, t1, t2) for t, lr in zip(self.trainers, learners)]

    def save(self, directory):
        """One npz checkpoint per member, seed_<seed>.npz under `directory`; the paths."""
        os.makedirs(directory, exist_ok=True)
        return [t.save(os.path.join(directory, f"seed_{s}.npz")) for t, s in zip(self.trainers, self.seeds)]

    def restore(self, directory):
        for t, s in zip(self.trainers, self.seeds):
            t.restore(os.path.join(directory, f"seed_{s}.npz"))

    def stop(self):
        if getattr(self, "rollout_group", None) is not None:   # before its members and their envs
            self.rollout_group.close()
            self.rollout_group = None
        self.noise = []
        if getattr(self, "finish_group", None) is not None:   # before its members
            self.finish_group.close()
            self.finish_group = None
        if self.group is not None:   # before its members
            self.group.close()
            self.group = None
        for t in self.trainers:
            t.stop()
        self.trainers = []
