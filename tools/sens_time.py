"""Timing of an evaluation env-step with the input-sensitivity kernel ("Sensitivity").

Centralized with a target velocity (d = 44, A = 8) and Local (4 policies, d = 35, A = 2) at
N = 128, over device-resident synthetic inputs, three ways on the same context:
  sens      ddrl_eval_act + ddrl_eval_sens + ddrl_eval_step
  launches  ddrl_eval_act + 2 d further ddrl_eval_act launches on pre-perturbed observation batches
            + ddrl_eval_step: the only route to the perturbed means without the kernel
  eval      ddrl_eval_act + ddrl_eval_step alone
and `sens` again with the kernel's grid capped (DDRL_SENS_GRID, read at every launch) so that a
workgroup takes 1, 2, 4 or 8 base rows with its weights staged once, also at N = 1024 (`sens`
itself runs the library's default cap).
Device events around windows of env-steps after a warm-up window, `--repeats` windows per variant,
the variants alternating; median and spread in microseconds per env-step.  Writes one JSON
document (default profiles/eval/sens_time.json).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddrl_amd import native as N
from ddrl_amd.spec import make_cfg

K = 8
CASES = {"centralized_tvel": ("QuantrupedMultiEnv_Centralized", {"env_config": {"target_velocity": [1.0]}}),
         "local": ("QuantrupedMultiEnv_Local", None)}


def make(env, config, n):
    cfg, _ = make_cfg(env, n, 8, config)
    ctx = N.Context(cfg, 0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(7)
    D = cfg.obs_full_dim
    for p in range(cfg.n_policies):
        ctx.params_set(p, (rng.normal(size=ctx.n_params[p]) * 0.05).astype(np.float32))
    ctx.filter_set(1000.0, rng.normal(size=D) * 0.1, np.abs(rng.normal(size=D)) * 999 + 1)
    return ctx, cfg


def inputs(n, cfg, d):
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    r = lambda *s: torch.randn(s, device="cuda", generator=g)
    D = cfg.obs_full_dim
    return dict(obs=r(K, n, D) * 2 + 0.5, pert=r(2 * d, n, D) * 2 + 0.5, fw=r(K, n), cfrc=r(K, n, 14, 6) * 1.5,
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


def time_case(env, config, n, steps, repeats, grids, with_launches):
    ctx, cfg = make(env, config, n)
    d = max(cfg.obs_dim[p] for p in range(cfg.n_policies))
    x = inputs(n, cfg, d)
    ctx.eval_begin(1 << 20, filter_update=False)   # a quota no env fills: every row accumulates at every step
    ctx.eval_sens_begin([np.full(cfg.obs_dim[p], 0.1) for p in range(cfg.n_policies)])

    def finish(k):
        ctx.eval_step(x["fw"][k], x["cfrc"][k], x["actions"], x["kin"][k], x["done"][k])

    def ev(i):
        k = i % K
        ctx.eval_act(x["obs"][k], None, x["actions"])
        finish(k)

    def sens(i):
        k = i % K
        ctx.eval_act(x["obs"][k], None, x["actions"])
        ctx.eval_sens(x["obs"][k])
        finish(k)

    def launches(i):
        k = i % K
        ctx.eval_act(x["obs"][k], None, x["actions"])
        for r in range(2 * d):
            ctx.eval_act(x["pert"][r], None, x["actions"])
        finish(k)

    def capped(g):
        def f(i):
            sens(i)
        f.grid = g
        return f

    variants = {"eval": (ev, steps), "sens": (sens, steps)}
    if with_launches:
        variants["launches"] = (launches, max(steps // 10, 20))
    for g in grids:
        variants[f"sens_grid{g}"] = (capped(g), steps)
    os.environ.pop("DDRL_SENS_GRID", None)

    def run(name, count):
        f, _ = variants[name]
        if getattr(f, "grid", None):
            os.environ["DDRL_SENS_GRID"] = str(f.grid)
        try:
            return window(f, count)
        finally:
            os.environ.pop("DDRL_SENS_GRID", None)

    for name, (_, count) in variants.items():   # warm-up: every kernel of every variant
        run(name, min(count, 100))
    t = {name: [] for name in variants}
    for _ in range(repeats):
        for name, (_, count) in variants.items():
            t[name].append(run(name, count))
    ctx.synchronize()
    rows = [ctx.eval_sens_results(p)[2] for p in range(cfg.n_policies)]
    ctx.eval_end()
    ctx.close()
    out = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in t.items()}
    out["sens_minus_eval_us"] = out["sens"]["median_us"] - out["eval"]["median_us"]
    if with_launches:
        out["launches_over_sens"] = out["launches"]["median_us"] / out["sens"]["median_us"]
    out["perturbed_rows_per_step"] = int(sum(2 * cfg.obs_dim[p] * ctx.layout[p]["C"] for p in range(cfg.n_policies)))
    out["base_rows_accumulated"] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "eval", "sens_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sens_time: needs a GPU (no timing without one)")
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit, "steps_per_window": a.steps,
           "repeats": a.repeats, "unit": "microseconds per env-step (all N envs), device events", "cases": {}}
    for name, (env, config) in CASES.items():
        res["cases"][name] = {
            "128": time_case(env, config, 128, a.steps, a.repeats, (128, 64, 32, 16), True),
            "1024": time_case(env, config, 1024, max(a.steps // 4, 50), a.repeats, (1024, 512, 256, 128), False)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
