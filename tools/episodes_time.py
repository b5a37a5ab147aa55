"""Timing of ddrl_episodes_collect against ddrl_gae ("Episode accounting").

Local at 4096 envs x 200 steps (the bench size), device-resident synthetic records and a done rate
of 1/200 per step.  Device events around each call, `--calls` calls after a warm-up, the two
alternating on one context in one session; a one-step reward call re-arms the fragment between
collects, outside the timed window.  collect = count + scan launches, one stream synchronize to
size the table, the walk launch; gae = k_gae + k_gae_finalize.  Median and spread in microseconds,
and their ratio.  Writes one JSON document (default profiles/episodes/episodes_time.json).
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out


def stats(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="QuantrupedMultiEnv_Local")
    ap.add_argument("--n-envs", type=int, default=4096)
    ap.add_argument("--frag-len", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "episodes", "episodes_time.json"))
    a = ap.parse_args(argv)
    n, T = a.n_envs, a.frag_len
    cfg, _ = make_cfg(a.env, n, T)
    ctx = N.Context(cfg, 0, torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    for p in range(cfg.n_policies):
        ctx.records_tensor(p).copy_(torch.randn(ctx.records_tensor(p).shape, device="cuda", generator=g))
    rng = np.random.default_rng(5)
    ctx.done_set((rng.random(size=(T, n)) < 1.0 / 200).astype(np.uint8))
    fw = torch.randn((n,), device="cuda", generator=g)
    cfrc = torch.randn((n, 14, 6), device="cuda", generator=g)
    actions = torch.rand((n, 8), device="cuda", generator=g) * 2 - 1
    done0 = torch.zeros((n,), dtype=torch.uint8, device="cuda")

    def rearm():
        ctx.reward(0, fw, cfrc, actions, done0)

    collect, gae, rows = [], [], []
    for i in range(a.warmup + a.calls):
        rearm()
        tc, r = timed(lambda: _collect(ctx))
        tg, _ = timed(ctx.gae)
        if i >= a.warmup:
            collect.append(tc)
            gae.append(tg)
            rows.append(r)
    ctx.synchronize()
    res = {"device": torch.cuda.get_device_name(0), "env": a.env, "n_envs": n, "frag_len": T, "calls": a.calls,
           "unit": "microseconds per call, device events",
           "episodes_per_collect": statistics.median(rows),
           "collect": stats(collect), "gae": stats(gae),
           "collect_over_gae": statistics.median(collect) / statistics.median(gae)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


def _collect(ctx):
    """ddrl_episodes_collect alone (no row copy): the count."""
    import ctypes as C
    nf = C.c_int64()
    N._ck(ctx.lib.ddrl_episodes_collect(ctx.h, C.byref(nf)))
    return int(nf.value)


if __name__ == "__main__":
    main()
