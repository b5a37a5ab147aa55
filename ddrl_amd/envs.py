"""Vectorized environment backends that feed the HIP rollout kernels.

SyntheticVecEnv is the synthetic QuAntruped used for the metric (MuJoCo is out of scope
and not installed): observations and rewards are seeded Gaussian draws generated on the
device each step, contact forces likewise, and episodes end every 1000 steps with
staggered phases (the gym TimeLimit of simulation_envs/__init__.py:27-32).  A MuJoCo
backend only has to implement the same reset()/step() on host cores and hand over pinned
buffers.

HostVecEnv and DeviceVecEnv run the QuAntruped stand-in on host threads and in a HIP kernel; both
take the ground's smoothness (env_config["hf_smoothness"]) and the adaptor's smoothness curriculum,
and their update_environment_after_epoch renews the ground as the reference's does.  The synthetic
env has no ground.
"""
from __future__ import annotations


class SyntheticVecEnv:
    def __init__(self, n_envs, obs_dim, device, seed=0, max_episode_steps=1000):
        import torch
        self.torch = torch
        self.N, self.D, self.device = n_envs, obs_dim, device
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(seed)
        self.max_steps = max_episode_steps
        self.t = torch.randint(0, max_episode_steps, (n_envs,), device=device, generator=self.gen)

    def _randn(self, *shape):
        return self.torch.randn(shape, device=self.device, generator=self.gen)

    def reset(self):
        return self._randn(self.N, self.D)

    def step(self, actions):
        self.t += 1
        done = (self.t % self.max_steps == 0).to(self.torch.uint8)
        obs = self._randn(self.N, self.D)
        return obs, self._randn(self.N), self._randn(self.N, 14, 6), done

    def update_environment_after_epoch(self, timesteps_total):
        """env.reset() of every env (quantruped_adaptor_multi_environment.py:97-122): the
        TimeLimit counts restart; no done flag, the next observation is the usual draw."""
        self.t.zero_()


class _TerrainMixin:
    """The env plane's terrain surface (native.HostEnv / DevEnv) on a trainer backend, and the
    adaptor's update_environment_after_epoch over it (quantruped_adaptor_multi_environment.py:97-122):
    with a curriculum, new smoothness bounds; in every case new ground (create_new_random_hfield),
    then env.reset() of every env."""

    curriculum = None   # (initial, target, last_timestep) when env_config sets curriculum_learning

    def set_terrain(self, lo, hi=None, bump_scale=2.0, generation=None):
        self.env.set_terrain(lo, hi, bump_scale, generation)

    @property
    def terrain(self):
        return self.env.terrain

    def new_terrain(self):
        self.env.new_terrain()

    def terrain_height(self, env_index, xy):
        return self.env.terrain_height(env_index, xy)

    def update_environment_after_epoch(self, timesteps_total):
        if self.curriculum is not None:
            lo, hi = curriculum_bounds(*self.curriculum, timesteps_total)
            self.env.set_terrain(lo, hi, self.env.terrain["bump_scale"])
        self.env.new_terrain()
        self.env.reset_state()


def curriculum_bounds(initial, target, last_timestep, timesteps_total):
    """The smoothness interval (lo, hi) of the reference's curriculum (adaptor :104-120), from which
    every env draws: while timesteps_total < last_timestep the lower bound moves linearly from the
    initial smoothness towards the target, lo = initial - (initial - target) * timesteps_total /
    last_timestep; afterwards lo = target.  hi = initial throughout.  (The reference draws one
    np.random.rand() per env inside that interval; here the env plane's hash does.)"""
    initial, target = float(initial), float(target)
    if last_timestep > timesteps_total:
        lo = initial - (initial - target) * (timesteps_total / last_timestep)
    else:
        lo = target
    return min(lo, initial), max(lo, initial)


def curriculum_of(env_config):
    """env_config's curriculum as (initial, target, last_timestep), or None without curriculum_learning."""
    if not env_config.get("curriculum_learning", False):
        return None
    if "range_smoothness" not in env_config or "range_last_timestep" not in env_config:
        raise ValueError("curriculum_learning needs range_smoothness [initial, target] and range_last_timestep")
    r = env_config["range_smoothness"]
    return float(r[0]), float(r[1]), float(env_config["range_last_timestep"])


class HostVecEnv(_TerrainMixin):
    """The host env plane (ddrl_amd.native.HostEnv: the QuAntruped stand-in stepped by a pool of
    host threads into pinned buffers) as a trainer backend: device tensors in and out, with a
    per-env target velocity drawn from the list on every reset (TVel envs) and the
    update_environment_after_epoch reset.  The bench's PCIe leg uses the same plane through
    the pipelined ddrl_rollout_hostenv instead."""

    def __init__(self, n_envs, obs_dim, device, seed=0, n_threads=4, target_velocity=0.0, hf_smoothness=1.0,
                 curriculum=None):
        import torch
        from .native import HostEnv
        self.torch, self.device = torch, device
        self.env = HostEnv(n_envs, obs_dim, n_threads, seed, target_velocity)
        self.env.set_terrain(hf_smoothness)
        self.curriculum = curriculum

    def _dev(self, a):
        return self.torch.from_numpy(a).to(self.device, non_blocking=False)

    def reset(self):
        return self._dev(self.env.reset())

    def step(self, actions):
        self.env.act[:] = actions.detach().to("cpu").numpy()
        self.env.step()
        return (self._dev(self.env.obs.copy()), self._dev(self.env.fw.copy()), self._dev(self.env.cfrc.copy()),
                self._dev(self.env.done.copy()))

    @property
    def target_velocities(self):
        return self.env.target_velocities

    def close(self):
        self.env.close()


class DeviceVecEnv(_TerrainMixin):
    """The device env plane (ddrl_amd.native.DevEnv: the same stand-in stepped by a HIP kernel on
    the rollout context's stream) as a trainer backend.  step() is one launch; what it returns are
    the plane's own device buffers, rewritten in place by the next step -- no host copy, no host
    thread, no synchronization."""

    def __init__(self, ctx, seed=0, target_velocity=0.0, hf_smoothness=1.0, curriculum=None):
        from .native import DevEnv
        self.env = DevEnv(ctx, seed, target_velocity)
        self.env.set_terrain(hf_smoothness)
        self.curriculum = curriculum

    def reset(self):
        return self.env.reset()

    def step(self, actions):
        self.env.step(actions)
        return self.env.obs, self.env.fw, self.env.cfrc, self.env.done

    @property
    def target_velocities(self):
        return self.env.target_velocities

    def close(self):
        self.env.close()
