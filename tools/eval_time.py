"""Timing of an evaluation env-step ("Evaluation").

Local, N = 128 and N = 4096, over device-resident synthetic inputs, two ways on the same context:
  eval      ddrl_eval_act + ddrl_eval_step (the fused evaluation forward and the accumulator)
  rollout   ddrl_observe + ddrl_act + ddrl_reward (the training rollout's step: the only way to
            get actions without the evaluation kernels)
each with the env-side filter frozen and updating.  Device events around windows of `--steps`
env-steps after a warm-up window, `--repeats` windows per variant, the variants alternating;
the median and the spread are reported in microseconds per env-step.  Also: ddrl_eval_hostenv
env-steps/s at N = 128 with 16 host threads (host clock around the call, which ends in a stream
synchronize).  Writes one JSON document (default profiles/eval/eval_time.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddrl_amd import native as N
from ddrl_amd.spec import make_cfg

ENV, T, K = "QuantrupedMultiEnv_Local", 8, 16


def make(n, filter_update):
    cfg, _ = make_cfg(ENV, n, T)
    cfg.filter_update = filter_update
    ctx = N.Context(cfg, 0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(7)
    for p in range(cfg.n_policies):
        ctx.params_set(p, (rng.normal(size=ctx.n_params[p]) * 0.05).astype(np.float32))
    ctx.filter_set(1000.0, rng.normal(size=43) * 0.1, np.abs(rng.normal(size=43)) * 999 + 1)
    return ctx, cfg


def inputs(n, cfg):
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    r = lambda *s: torch.randn(s, device="cuda", generator=g)
    return dict(obs=r(K, n, 43) * 2 + 0.5, eps=r(K, n, cfg.n_agents, cfg.act_dim), fw=r(K, n), cfrc=r(K, n, 14, 6) * 1.5,
                kin=r(K, n, 9), done=(torch.rand((K, n), device="cuda", generator=g) < 0.01).to(torch.uint8),
                actions=torch.zeros((n, 8), device="cuda"))


def window(step, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        step(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps   # us per env-step


def time_shape(n, steps, repeats):
    out = {}
    for mode, upd in (("frozen", 0), ("updating", 1)):
        ctx, cfg = make(n, upd)
        x = inputs(n, cfg)
        ctx.eval_begin(4, filter_update=bool(upd))   # envs past their quota still accumulate and restart

        def ev(i):
            k = i % K
            ctx.eval_act(x["obs"][k], x["eps"][k], x["actions"])
            ctx.eval_step(x["fw"][k], x["cfrc"][k], x["actions"], x["kin"][k], x["done"][k])

        def ro(i):
            k = i % K
            ctx.observe(x["obs"][k])
            ctx.act(i % T, x["eps"][k], x["actions"])
            ctx.reward(i % T, x["fw"][k], x["cfrc"][k], x["actions"], x["done"][k])

        for f in (ev, ro):   # warm-up: every kernel of both variants
            window(f, min(steps, 200))
        t = {"eval": [], "rollout": []}
        for _ in range(repeats):
            t["eval"].append(window(ev, steps))
            t["rollout"].append(window(ro, steps))
        ctx.synchronize()
        ctx.eval_end()
        ctx.close()
        for k, v in t.items():
            out[f"{k}_{mode}"] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
        out[f"ratio_{mode}"] = out[f"rollout_{mode}"]["median_us"] / out[f"eval_{mode}"]["median_us"]
    return out


def time_hostenv(n, threads, steps):
    ctx, cfg = make(n, 1)
    env = N.HostEnv(n, 43, n_threads=threads, seed=1)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    eps = torch.randn((steps, n, cfg.n_agents, cfg.act_dim), device="cuda", generator=g)
    ctx.eval_begin(steps, filter_update=True)   # a quota no env fills: the loop runs every step
    ctx.eval_hostenv(env, eps, steps, min(steps, 200), poll_every=25)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ran = ctx.eval_hostenv(env, eps, steps, steps, poll_every=25)
    dt = time.perf_counter() - t0
    ctx.eval_end()
    ctx.close()
    env.close()
    return {"n_envs": n, "host_threads": threads, "steps": ran, "seconds": dt, "env_steps_per_s": ran * n / dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "eval", "eval_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_time: needs a GPU (no timing without one)")
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit, "env": ENV, "steps_per_window": a.steps,
           "repeats": a.repeats, "unit": "microseconds per env-step (all N envs), device events",
           "shapes": {str(n): time_shape(n, a.steps, a.repeats) for n in (128, 4096)},
           "eval_hostenv": time_hostenv(128, 16, a.steps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
