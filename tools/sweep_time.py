"""Timing of the evaluation members ("Evaluation members").

Local, in one session, every variant after a warm-up, `--repeats` windows per variant, the variants
alternating; medians and spreads (min .. max over the windows) are reported.
  act        microseconds per ddrl_eval_act call in member mode at (M, n) = (1, 128), (16, 8),
             (128, 8) and (210, 10), filter frozen and continuing, each against the plain
             ddrl_eval_act of a context of the same M * n envs in the same run (device events
             around windows of `--steps` calls over rotating observation buffers).  The plain
             kernels are the parent's, unchanged: they are the baseline.
  sweep      PPOTrainer.evaluate_members of 16 members x 8 envs x 1 episode x 200 steps against 16
             sequential evaluate(env_backend="device", n_envs=8) calls in the same process (host
             clock around the calls, which end synchronized with their results on the host).  The
             members are the trainer's current state: no checkpoint file is read in either variant.
  step       with --parent-root DIR (a built checkout of the parent commit): the flat
             k_devenv_step launch of this tree (per-env velocity table unset) against the parent's,
             by tools/devenv_time.py --terrain --parent-root (child processes, alternating).
Writes one JSON document (default profiles/eval/sweep_time.json).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from ddrl_amd import native as N
from ddrl_amd.spec import make_cfg

ENV, K = "QuantrupedMultiEnv_Local", 16
SHAPES = [(1, 128), (16, 8), (128, 8), (210, 10)]


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def window(step, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        step(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps   # us per call


def alternate(variants, run, repeats):
    for name in variants:
        run(name)
    out = {name: [] for name in variants}
    for _ in range(repeats):
        for name in variants:
            out[name].append(run(name))
    return {name: summary(v) for name, v in out.items()}


def make(n_envs):
    cfg, _ = make_cfg(ENV, n_envs, 1)
    ctx = N.Context(cfg, 0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(7)
    for p in range(cfg.n_policies):
        ctx.params_set(p, (rng.normal(size=ctx.n_params[p]) * 0.05).astype(np.float32))
    ctx.filter_set(1000.0, rng.normal(size=43) * 0.1, np.abs(rng.normal(size=43)) * 999 + 1)
    return ctx, cfg


def time_act(M, n, steps, repeats):
    out = {}
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    Nn = M * n
    obs = torch.randn((K, Nn, 43), device="cuda", generator=g)
    for mode, upd in (("frozen", False), ("continuing", True)):
        ctxs = {}
        for name in ("members", "plain"):
            ctx, cfg = make(Nn)
            ctx.eval_begin(1, filter_update=upd)
            if name == "members":
                ctx.eval_members_begin(M)
                for m in range(M):
                    ctx.eval_member_load(m)
            ctxs[name] = ctx
        eps = torch.randn((K, Nn, cfg.n_agents, cfg.act_dim), device="cuda", generator=g)
        actions = torch.zeros((Nn, 8), device="cuda")
        res = alternate(["members", "plain"],
                        lambda name: window(lambda i: ctxs[name].eval_act(obs[i % K], eps[i % K], actions), steps),
                        repeats)
        spread = max(res[k]["max"] - res[k]["min"] for k in res)
        gap = res["members"]["median"] - res["plain"]["median"]
        out[mode] = {**res, "members_minus_plain": gap, "spread": spread,
                     "members_slower_by_more_than_spread": bool(gap > spread)}
        for ctx in ctxs.values():
            ctx.synchronize()
            ctx.eval_end()
            ctx.close()
    return {"members": M, "envs_per_member": n, "unit": "microseconds per ddrl_eval_act call (all M * n envs)", **out}


def time_sweep(repeats, members=16, n=8, num_steps=200):
    from ddrl_amd.trainer import PPOTrainer
    tr = PPOTrainer({"env": ENV, "rollout_fragment_length": 8}, n_envs=8, seed=1)
    args = dict(num_episodes=n, num_steps=num_steps, explore=True, seed=3)

    def run(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "evaluate_members":
            res = tr.evaluate_members([(None, None)] * members, **args)
            rows = sum(len(r[0]) for r in res)
        else:
            rows = sum(len(tr.evaluate(env_backend="device", n_envs=n, **args)[0]) for _ in range(members))
        dt = time.perf_counter() - t0
        assert rows == members * n, rows
        return dt * 1e3
    res = alternate(["evaluate_members", "sequential_evaluate"], run, repeats)
    tr.stop()
    return {"members": members, "envs_per_member": n, "episodes_per_env": 1, "num_steps": num_steps,
            "unit": "milliseconds per sweep (host clock, results on the host)", **res,
            "sequential_over_members": res["sequential_evaluate"]["median"] / res["evaluate_members"]["median"]}


def time_step_vs_parent(a, out_dir):
    path = os.path.join(out_dir, "sweep_step_vs_parent.json")
    cmd = [sys.executable, os.path.join(HERE, "tools", "devenv_time.py"), "--terrain", "--parent-root",
           os.path.abspath(a.parent_root), "--rounds", str(a.rounds), "--steps", str(a.steps), "--repeats",
           str(a.repeats), "--out", path]
    r = subprocess.run(cmd, timeout=1500)   # its progress lines go to this process's output
    if r.returncode != 0:
        sys.exit("sweep_time: tools/devenv_time.py failed")
    with open(path) as f:
        doc = json.load(f)
    os.remove(path)
    keep = ("flat", "parent_flat", "flat_within_parent_spread", "flat_minus_parent_flat")
    return {"unit": "microseconds per k_devenv_step launch, flat ground, velocity table unset; medians of "
                    f"{a.rounds} processes per tree",
            **{k: {f: v[f] for f in keep} for k, v in doc["summary"].items() if k.startswith("step_")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="--parent-root: processes per tree")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit (the step figure)")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "eval", "sweep_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sweep_time: needs a GPU (no timing without one)")
    out_dir = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit, "env": ENV, "calls_per_window": a.steps,
           "repeats": a.repeats,
           "act": {f"{M}x{n}": time_act(M, n, a.steps, a.repeats) for M, n in SHAPES},
           "sweep": time_sweep(a.repeats)}
    if a.parent_root:
        res["step"] = time_step_vs_parent(a, out_dir)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
