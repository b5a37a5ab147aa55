"""Timing of the device env plane ("Device env plane").

Local, in one session, every variant after a warm-up, `--repeats` windows per variant, the
variants alternating; medians and spreads are reported.
  step      microseconds per k_devenv_step launch at N = 128 and 4096 (device events around
            windows of `--steps` launches over rotating action buffers)
  eval      the evaluation env step over the device plane (ddrl_eval_act + ddrl_devenv_step +
            ddrl_eval_step) at N = 128 and 4096, filter frozen and updating (device events); and
            ddrl_eval_devenv against ddrl_eval_hostenv (16 host threads) at N = 128 in env-steps/s
            (host clock around the calls, which end synchronized)
  fragment  a T = 200 fragment at 4096 envs: ddrl_rollout_devenv against ddrl_rollout_hostenv
            (8 groups, 16 host threads) and ddrl_rollout_fragment over synthetic buffers (host
            clock around call + synchronize), in env-steps/s
Writes one JSON document (default profiles/devenv/devenv_time.json).

  --terrain  the cost of uneven ground (profiles/devenv/terrain_time.json): the step launch at
            N = 128 and 4096 and the T = 200 fragment at 4096 envs, flat and with smoothness 0.6
            (the fragment also with a new_terrain before every call, which captures the loop
            again), the variants alternating inside a process.  With --parent-root DIR (a built
            checkout of the parent commit) the same flat figures are taken from that tree too, in
            child processes of this one that alternate with this tree's, `--rounds` times each;
            the verdict says whether this tree's flat medians lie inside the parent's
            run-to-run spread (min .. max over its rounds).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --root DIR: the tree whose ddrl_amd package (and library) is measured; this one by default
ROOT = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else HERE
sys.path.insert(0, os.path.abspath(ROOT))
from ddrl_amd import native as N
from ddrl_amd.spec import make_cfg

ENV, K = "QuantrupedMultiEnv_Local", 16


def make(n, T, filter_update=1):
    cfg, _ = make_cfg(ENV, n, T)
    cfg.filter_update = filter_update
    ctx = N.Context(cfg, 0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(7)
    for p in range(cfg.n_policies):
        ctx.params_set(p, (rng.normal(size=ctx.n_params[p]) * 0.05).astype(np.float32))
    ctx.filter_set(1000.0, rng.normal(size=43) * 0.1, np.abs(rng.normal(size=43)) * 999 + 1)
    return ctx, cfg


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def window(step, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        step(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps   # us per step


def alternate(variants, run, repeats):
    """run(name) -> one figure; every variant warmed up, then `repeats` rounds over all of them."""
    for name in variants:
        run(name)
    out = {name: [] for name in variants}
    for _ in range(repeats):
        for name in variants:
            out[name].append(run(name))
    return {name: summary(v) for name, v in out.items()}


def time_step(n, steps, repeats):
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    actions = torch.rand((K, n, 8), device="cuda", generator=g) * 2 - 1
    ctx, cfg = make(n, 8)
    env = N.DevEnv(ctx, seed=1)
    env.reset()
    res = alternate(["step"], lambda name: window(lambda i: env.step(actions[i % K]), steps), repeats)
    env.close()
    ctx.close()
    return {"unit": "microseconds per launch", **res["step"]}


def time_eval_step(n, steps, repeats):
    out = {}
    for mode, upd in (("frozen", 0), ("updating", 1)):
        ctx, cfg = make(n, 8, upd)
        env = N.DevEnv(ctx, seed=1)
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        eps = torch.randn((K, n, cfg.n_agents, cfg.act_dim), device="cuda", generator=g)
        actions = torch.zeros((n, 8), device="cuda")
        ctx.eval_begin(1 << 20, filter_update=bool(upd))   # a quota no env fills
        env.reset_episodes()

        def ev(i):
            ctx.eval_act(env.obs, eps[i % K], actions)
            env.step(actions)
            ctx.eval_step(env.fw, env.cfrc, actions, env.kin, env.done)
        out[mode] = alternate(["eval_step"], lambda name: window(ev, steps), repeats)["eval_step"]
        ctx.synchronize()
        ctx.eval_end()
        env.close()
        ctx.close()
    return {"unit": "microseconds per env-step (all N envs)", **out}


def time_eval_loops(n, threads, steps, repeats):
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    planes = {}
    for name in ("device", "host"):
        ctx, cfg = make(n, 8)
        env = N.DevEnv(ctx, seed=1) if name == "device" else N.HostEnv(n, 43, n_threads=threads, seed=1)
        ctx.eval_begin(steps, filter_update=True)   # a quota no env fills: the loop runs every step
        planes[name] = (ctx, env)
    eps = torch.randn((steps, n, 4, 2), device="cuda", generator=g)

    def run(name):
        ctx, env = planes[name]
        loop = ctx.eval_devenv if name == "device" else ctx.eval_hostenv
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ran = loop(env, eps, steps, steps, poll_every=25)
        ctx.synchronize()
        return ran * n / (time.perf_counter() - t0)
    res = alternate(["device", "host"], run, repeats)
    for ctx, env in planes.values():
        ctx.eval_end()
        env.close()
        ctx.close()
    return {"n_envs": n, "host_threads": threads, "steps": steps, "unit": "env-steps per second", **verdict(res)}


def verdict(res):
    """device against host: the gap in units of the host numbers' run-to-run spread."""
    spread = res["host"]["max"] - res["host"]["min"]
    gap = res["device"]["median"] - res["host"]["median"]
    return {**res, "host_spread": spread, "device_minus_host": gap,
            "device_over_host": res["device"]["median"] / res["host"]["median"],
            "faster_by_more_than_5_spreads": bool(gap > 5 * spread)}


def time_fragments(n, T, groups, threads, repeats):
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    r = lambda *s: torch.randn(s, device="cuda", generator=g)
    ctxs = {name: make(n, T)[0] for name in ("device", "host", "synthetic")}
    cfg = ctxs["device"].cfg
    eps = r(T, n, cfg.n_agents, cfg.act_dim)
    denv = N.DevEnv(ctxs["device"], seed=1)
    henv = N.HostEnv(n, 43, n_threads=threads, seed=1)
    syn = dict(obs=r(T + 1, n, 43), fw=r(T, n), cfrc=r(T, n, 14, 6),
               done=(torch.rand((T, n), device="cuda", generator=g) < 0.001).to(torch.uint8),
               actions=torch.zeros((n, 8), device="cuda"))
    ctxs["device"].rollout_devenv(denv, eps, reset=True)
    ctxs["host"].rollout_hostenv(henv, eps, groups=groups, reset=True)
    ctxs["synthetic"].observe(syn["obs"][0])

    def run(name):
        ctx = ctxs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "device":
            ctx.rollout_devenv(denv, eps)
        elif name == "host":
            ctx.rollout_hostenv(henv, eps, groups=groups)
        else:
            ctx.rollout_fragment(syn["obs"], eps, syn["fw"], syn["cfrc"], syn["done"], syn["actions"])
        ctx.synchronize()
        return n * T / (time.perf_counter() - t0)
    res = alternate(["device", "host", "synthetic"], run, repeats)
    denv.close()
    henv.close()
    for c in ctxs.values():
        c.close()
    us = {name: 1e6 * n / v["median"] for name, v in res.items()}   # per env step of the fragment
    return {"n_envs": n, "T": T, "groups": groups, "host_threads": threads, "unit": "env-steps per second",
            **verdict(res), "us_per_step": us, "device_minus_synthetic_us_per_step": us["device"] - us["synthetic"]}


SMOOTH = 0.6


def time_terrain_step(n, steps, repeats):
    """The step launch, flat and on uneven ground (the envs spread over x = 5 .. 45 m, off the start
    patch); a tree without terrain gives the flat figure only."""
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    actions = torch.rand((K, n, 8), device="cuda", generator=g) * 2 - 1
    ctx, cfg = make(n, 8)
    env = N.DevEnv(ctx, seed=1)
    env.reset()
    st = env.state()
    st[:, 0] = np.linspace(5.0, 45.0, n)
    env.set_state(st)
    variants = ["flat"] + (["terrain"] if hasattr(env, "set_terrain") else [])

    def run(name):
        if len(variants) > 1:
            env.set_terrain(SMOOTH if name == "terrain" else 1.0)
        return window(lambda i: env.step(actions[i % K]), steps)
    res = alternate(variants, run, repeats)
    env.close()
    ctx.close()
    return {"unit": "microseconds per launch", **res}


def time_terrain_fragment(n, T, repeats):
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    ctx, cfg = make(n, T)
    eps = torch.randn((T, n, cfg.n_agents, cfg.act_dim), device="cuda", generator=g)
    env = N.DevEnv(ctx, seed=1)
    ctx.rollout_devenv(env, eps, reset=True)
    has = hasattr(env, "set_terrain")
    variants = ["flat"] + (["terrain", "terrain_renewed"] if has else [])

    def run(name):
        if has:
            env.set_terrain(SMOOTH if name != "flat" else 1.0)
            ctx.rollout_devenv(env, eps)      # the capture of this variant's loop is not in the window
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "terrain_renewed":
            env.new_terrain()                 # what update_environment_after_epoch does: the loop is captured again
        ctx.rollout_devenv(env, eps)
        ctx.synchronize()
        return 1e6 * (time.perf_counter() - t0) / T
    res = alternate(variants, run, repeats)
    env.close()
    ctx.close()
    return {"n_envs": n, "T": T, "unit": "microseconds per env-step of the fragment (all N envs)", **res}


def terrain_worker(a):
    return {"step": {str(n): time_terrain_step(n, a.steps, a.repeats) for n in (128, 4096)},
            "fragment": time_terrain_fragment(4096, 200, a.repeats)}


def terrain_main(a):
    """This tree and, with --parent-root, the parent's, alternating in child processes."""
    import subprocess
    trees = {"this": HERE}
    if a.parent_root:
        trees["parent"] = os.path.abspath(a.parent_root)
    rounds = {name: [] for name in trees}
    device = ""
    for _ in range(a.rounds):
        for name, root in trees.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--terrain-worker", "--root", root,
                                  "--steps", str(a.steps), "--repeats", str(a.repeats)],
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                sys.exit(f"devenv_time: the {name} tree's worker failed:\n{out.stderr[-2000:]}")
            doc = json.loads(out.stdout.strip().splitlines()[-1])
            device = doc.pop("device")
            rounds[name].append(doc)
            print(name, json.dumps(doc), flush=True)

    def node(doc, path):
        for k in path:
            doc = doc[k]
        return doc

    def medians(name, *path):
        return [node(doc, path)["median"] for doc in rounds[name]]
    keys = [("step", "128"), ("step", "4096"), ("fragment",)]
    res = {"device": device, "commit": a.commit, "env": ENV, "smoothness": SMOOTH, "steps_per_window": a.steps,
           "repeats_per_process": a.repeats, "processes_per_tree": a.rounds, "rounds": rounds, "summary": {}}
    for path in keys:
        first = node(rounds["this"][0], path)
        entry = {v: summary(medians("this", *path, v)) for v in first if isinstance(first[v], dict)}
        if "terrain" in entry:
            entry["terrain_minus_flat"] = entry["terrain"]["median"] - entry["flat"]["median"]
        if "parent" in rounds:
            par = summary(medians("parent", *path, "flat"))
            entry["parent_flat"] = par
            entry["flat_within_parent_spread"] = bool(par["min"] <= entry["flat"]["median"] <= par["max"])
            entry["flat_minus_parent_flat"] = entry["flat"]["median"] - par["median"]
        res["summary"]["_".join(path)] = entry
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE, help="the tree whose package is measured")
    ap.add_argument("--terrain", action="store_true", help="the terrain case only (see the module docstring)")
    ap.add_argument("--terrain-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parent-root", default="", help="--terrain: a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3, help="--terrain: processes per tree")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "devenv", "devenv_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("devenv_time: needs a GPU (no timing without one)")
    if a.terrain_worker:
        print(json.dumps({"device": torch.cuda.get_device_name(0), **terrain_worker(a)}))
        return
    if a.terrain:
        res = terrain_main(a)
        out = a.out if "--out" in sys.argv else os.path.join(HERE, "profiles", "devenv", "terrain_time.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["summary"]))
        return
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit, "env": ENV, "steps_per_window": a.steps,
           "repeats": a.repeats,
           "step": {str(n): time_step(n, a.steps, a.repeats) for n in (128, 4096)},
           "eval_step": {str(n): time_eval_step(n, a.steps, a.repeats) for n in (128, 4096)},
           "eval_loop": time_eval_loops(128, 16, a.steps, a.repeats),
           "fragment": time_fragments(4096, 200, 8, 16, a.repeats)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
