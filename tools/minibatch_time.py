"""Time per step of the fused PPO update at sgd_minibatch_size 128 and 256 (DESIGN.md section 3,
"256-row minibatches").

Two context shapes, T = 200: Local 4096 envs (4 independent leg policies, d = 35) and
SharedDecentral 1024 envs (one shared leg policy, d = 19); both hold 819,200 rows per policy.
Three variants per shape, each with a context of its own over the same seeded rollout:
  parent128   this size in the parent commit's library (--parent-lib: that commit's
              libddrl_hip.so, built from its tree and copied next to this one; default
              ddrl_amd/libddrl_hip_parent.so) -- the 128 figure the comparison uses,
  new128      the same in this tree's library (no 128 code changed: it must agree),
  new256      sgd_minibatch_size 256 in this tree's library,
  parent256   (--parent-256) sgd_minibatch_size 256 in the parent commit's library: the A/B of a
              change to the 256-row kernels themselves.
Device events around whole launches (ddrl_ppo_update of the full 10-epoch schedule), one
warm-up launch per variant, then --repeats launches per variant with the variants alternating;
every launch starts from the same weights and Adam state.  Reported: the median and the spread
in microseconds per step, rows per microsecond, the SHA-256 of theta after the last launch (equal
between variants of one size that claim the same arithmetic), and the cost of one 256-row step
against two 128-row steps of the parent library.  Writes profiles/minibatch/minibatch_time.json.

    python tools/minibatch_time.py [--repeats 5] [--parent-lib PATH | --no-parent] [--parent-256]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ddrl_amd import native as N
from ddrl_amd.spec import make_cfg
from ddrl_amd.synthetic import SyntheticRollout
from ddrl_amd.trainer import glorot_ffn_flat

T = 200
SHAPES = [("local", "QuantrupedMultiEnv_Local", 4096), ("c4", "QuantrupedMultiEnv_SharedDecentral", 1024)]


def use_library(path):
    """Contexts made from here on run `path` (a context keeps the library it was made with)."""
    N._lib = None
    return N.load(path)


class Variant:
    def __init__(self, lib_path, env, n, mb):
        use_library(lib_path)
        cfg, _ = make_cfg(env, n, T, {"sgd_minibatch_size": mb})
        self.ctx = ctx = N.Context(cfg, 0, torch.cuda.current_stream().cuda_stream)
        self.P, self.mb = cfg.n_policies, mb
        rng = np.random.default_rng(1234)
        self.theta = [glorot_ffn_flat(rng, cfg.obs_dim[p], cfg.act_dim) for p in range(self.P)]
        self.reset()
        syn = SyntheticRollout(n, T, cfg.obs_full_dim, cfg.n_agents, cfg.act_dim, "cuda:0", seed=0)
        ctx.observe(syn.obs[0])
        ctx.rollout_fragment(syn.obs, syn.eps, syn.fw, syn.cfrc, syn.dones_for_fragment(), syn.actions)
        ctx.gae()
        ctx.synchronize()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(99)
        R = T * ctx.layout[0]["C"]
        self.nb, E = R // mb, cfg.num_sgd_iter
        self.steps = E * self.nb
        self.sh = [torch.randperm(R, device="cuda", generator=gen, dtype=torch.int32) for _ in range(self.P)]
        self.pe = [torch.stack([torch.randperm(self.nb, device="cuda", generator=gen, dtype=torch.int32)
                                for _ in range(E)]).contiguous() for _ in range(self.P)]

    def reset(self):
        for p, th in enumerate(self.theta):
            self.ctx.params_set(p, th)
            self.ctx.adam_set(p, np.zeros(th.size, np.float32), np.zeros(th.size, np.float32), 0.9, 0.999)

    def launch_us_per_step(self):
        self.reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self.ctx.ppo_update((1 << self.P) - 1, self.sh, self.pe, [0.2] * self.P)
        b.record()
        b.synchronize()
        self.ctx.synchronize()   # raises if the launch failed
        return a.elapsed_time(b) * 1e3 / self.steps


def time_shape(env, n, repeats, libs):
    variants = {name: Variant(path, env, n, mb) for name, (path, mb) in libs.items()}
    for v in variants.values():
        v.launch_us_per_step()   # warm-up
    t = {name: [] for name in variants}
    for _ in range(repeats):
        for name, v in variants.items():
            t[name].append(v.launch_us_per_step())
    out = {}
    for name, v in variants.items():
        med = statistics.median(t[name])
        out[name] = {"sgd_minibatch_size": v.mb, "steps_per_launch": v.steps, "median_us_per_step": med,
                     "min_us_per_step": min(t[name]), "max_us_per_step": max(t[name]),
                     "us_per_step": t[name], "rows_per_us": v.mb / med, "launch_ms": med * v.steps * 1e-3,
                     "theta_sha256": hashlib.sha256(b"".join(v.ctx.params_get(p).tobytes()
                                                             for p in range(v.P))).hexdigest()[:16]}
        v.ctx.close()
    base = out.get("parent128", out["new128"])
    out["base_128"] = "parent128" if "parent128" in out else "new128"
    out["us_256_step_over_two_128_steps"] = out["new256"]["median_us_per_step"] / (2 * base["median_us_per_step"])
    out["rows_per_us_256_over_128"] = out["new256"]["rows_per_us"] / base["rows_per_us"]
    out["one_256_step_costs_less_than_two_128_steps"] = out["us_256_step_over_two_128_steps"] < 1.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=os.path.join(os.path.dirname(N.LIB_PATH), "libddrl_hip_parent.so"))
    ap.add_argument("--no-parent", action="store_true", help="compare against this tree's 128-row kernels only")
    ap.add_argument("--parent-256", action="store_true", help="also time the parent library's 256-row step")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minibatch", "minibatch_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("minibatch_time: needs a GPU (no timing without one)")
    libs = {}
    if not a.no_parent:
        if not os.path.exists(a.parent_lib):
            sys.exit(f"minibatch_time: {a.parent_lib} is missing: build the parent commit's library and copy it "
                     "there (or pass --no-parent)")
        libs["parent128"] = (a.parent_lib, 128)
    libs["new128"] = (N.LIB_PATH, 128)
    libs["new256"] = (N.LIB_PATH, 256)
    if a.parent_256 and not a.no_parent:
        libs["parent256"] = (a.parent_lib, 256)
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit, "frag_len": T, "repeats": a.repeats,
           "unit": "microseconds per minibatch step (all policies of the launch side by side), device events "
                   "around whole 10-epoch launches, variants alternating",
           "shapes": {key: {"env": env, "n_envs": n, **time_shape(env, n, a.repeats, libs)} for key, env, n in SHAPES}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
