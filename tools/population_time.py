"""Timing of the group update ("Population update").

One session, device events around whole update calls after a warm-up, three alternating runs of
each variant per size:
  group       one UpdateGroup.run of M members (snapshots, table copy, outbox clear and the launch);
  sequential  the same M updates issued one after the other through ddrl_ppo_update.
Reported per M: milliseconds per call, microseconds per minibatch step of the group launch (every
chain takes that step at once), aggregate minibatch rows per microsecond (M x P x 128 / step time),
the sequential updates' step time per member, and whether the group beat the sequential updates in
every run by more than the solo step's run-to-run spread.
  Local, 4096 envs x 200 steps (about 0.63 GB of records per member), M = 1, 2, 4, 8, 16: the whole
    10-epoch schedule (64,000 steps).
  C4 (SharedDecentral), 4096 envs, M = 1, 8, 64: capped at one epoch (25,600 steps) -- 64 sequential
    whole updates would take 160 s per run.
  solo regression, with --parent-root DIR (a built checkout of the parent commit): the solo
    ddrl_ppo_update of Local 4096 on this tree and on the parent's, child processes, alternating.
Writes one JSON document (default profiles/population/population_time.json).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCAL, C4 = "QuantrupedMultiEnv_Local", "QuantrupedMultiEnv_SharedDecentral"


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def make_members(N, make_cfg, env, n_envs, T, M):
    """M contexts with their own weights and a rolled-out, postprocessed fragment each."""
    import numpy as np
    import torch
    from ddrl_amd.trainer import glorot_ffn_flat
    from ddrl_amd.synthetic import SyntheticRollout
    cfg, _ = make_cfg(env, n_envs, T)
    syn = SyntheticRollout(n_envs, T, cfg.obs_full_dim, cfg.n_agents, cfg.act_dim, "cuda:0", seed=5)
    dones = syn.dones_for_fragment()
    ctxs = []
    for m in range(M):
        ctx = N.Context(cfg, 0, torch.cuda.current_stream().cuda_stream)
        rng = np.random.default_rng(100 + m)
        for p in range(cfg.n_policies):
            ctx.params_set(p, glorot_ffn_flat(rng, cfg.obs_dim[p], cfg.act_dim))
        ctx.observe(syn.obs[0])
        ctx.rollout_fragment(syn.obs, syn.eps, syn.fw, syn.cfrc, dones, syn.actions)
        ctx.gae()
        ctx.synchronize()
        ctxs.append(ctx)
    return ctxs, cfg


def schedule(ctx, T, seed):
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    sh, pe = [], []
    for p in range(ctx.cfg.n_policies):
        R = T * ctx.layout[p]["C"]
        sh.append(torch.from_numpy(rng.permutation(R).astype(np.int32)).cuda())
        pe.append(torch.from_numpy(np.stack([rng.permutation(R // 128) for _ in range(ctx.cfg.num_sgd_iter)])
                                   .astype(np.int32)).cuda())
    return sh, pe, [0.2] * ctx.cfg.n_policies


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)   # ms


def time_size(N, make_cfg, env, n_envs, T, M, max_steps, repeats, rel_spread):
    ctxs, cfg = make_members(N, make_cfg, env, n_envs, T, M)
    P = cfg.n_policies
    scheds = [schedule(c, T, 10 + m) for m, c in enumerate(ctxs)]
    group = N.UpdateGroup(ctxs)
    total = cfg.num_sgd_iter * (T * ctxs[0].layout[0]["C"] // 128)
    steps = total if max_steps < 0 else min(total, max_steps)
    mask = (1 << P) - 1

    def run_group(k):
        ms = timed(lambda: group.run([s[0] for s in scheds], [s[1] for s in scheds], [s[2] for s in scheds], k))
        group.finish()
        return ms

    def run_seq(k):
        ms = timed(lambda: [c.ppo_update(mask, s[0], s[1], s[2], max_steps=k) for c, s in zip(ctxs, scheds)])
        for c in ctxs:
            c.synchronize()
        return ms
    run_group(256)   # warm-up: code objects, clocks, the arenas' first touch
    run_seq(256)
    g, q = [], []
    for _ in range(repeats):
        g.append(run_group(max_steps))
        q.append(run_seq(max_steps))
    xcc = group.placement()
    group.close()
    for c in ctxs:
        c.close()
    us = [x * 1e3 / steps for x in g]
    res = {"members": M, "chains": M * P, "steps_per_update": steps, "group_ms": g, "sequential_ms": q,
           "group_us_per_step": summary(us),
           "aggregate_rows_per_us": M * P * 128 / statistics.median(us),
           "sequential_us_per_step_per_member": summary([x * 1e3 / steps / M for x in q]),
           "sequential_over_group": [b / a for a, b in zip(g, q)],
           "blocks": int(xcc.size)}
    if rel_spread is not None:
        res["group_wins_every_run_by_more_than_solo_spread"] = bool(all(b - a > rel_spread * b for a, b in zip(g, q)))
    print(json.dumps(res), flush=True)
    return res


def solo_child(root, n_envs, T, repeats):
    """Child process: the solo ddrl_ppo_update of Local on the tree at `root`; one JSON line."""
    sys.path.insert(0, root)
    import torch
    from ddrl_amd import native as N
    from ddrl_amd.spec import make_cfg
    ctxs, cfg = make_members(N, make_cfg, LOCAL, n_envs, T, 1)
    ctx, (sh, pe, kl) = ctxs[0], schedule(ctxs[0], T, 10)
    steps = cfg.num_sgd_iter * (T * ctx.layout[0]["C"] // 128)

    def run(k):
        ms = timed(lambda: ctx.ppo_update(15, sh, pe, kl, max_steps=k))
        ctx.synchronize()
        return ms
    run(256)
    print(json.dumps({"device": torch.cuda.get_device_name(0),
                      "us_per_step": [run(-1) * 1e3 / steps for _ in range(repeats)]}))


def solo_regression(a):
    out = {"this": [], "parent": []}
    for _ in range(a.rounds):
        for name, root in (("this", HERE), ("parent", os.path.abspath(a.parent_root))):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--solo-child", root, "--envs", str(a.envs),
                                "--frag-len", str(a.frag_len), "--repeats", str(a.repeats)],
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"population_time: the solo child of {root} failed:\n{r.stderr[-2000:]}")
            out[name] += json.loads(r.stdout.strip().splitlines()[-1])["us_per_step"]
    res = {"unit": "microseconds per step of the solo ddrl_ppo_update, Local, whole schedule; "
                   f"{a.rounds} alternating processes per tree x {a.repeats} updates",
           "this": summary(out["this"]), "parent": summary(out["parent"])}
    spread = res["parent"]["max"] - res["parent"]["min"]
    res["parent_spread"] = spread
    res["this_minus_parent"] = res["this"]["median"] - res["parent"]["median"]
    res["within_parent_spread"] = bool(abs(res["this_minus_parent"]) <= spread)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--frag-len", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="--parent-root: processes per tree")
    ap.add_argument("--local", default="1,2,4,8,16", help="member counts of the Local size ('' skips it)")
    ap.add_argument("--c4", default="1,8,64", help="member counts of the C4 size ('' skips it)")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit (the solo regression)")
    ap.add_argument("--solo-child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "population", "population_time.json"))
    a = ap.parse_args()
    if a.solo_child:
        return solo_child(a.solo_child, a.envs, a.frag_len, a.repeats)
    sys.path.insert(0, HERE)
    import torch
    from ddrl_amd import native as N
    from ddrl_amd.spec import make_cfg
    if not torch.cuda.is_available():
        sys.exit("population_time: needs a GPU (no timing without one)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit, "envs": a.envs, "frag_len": a.frag_len,
           "repeats": a.repeats}
    rel = None
    if a.parent_root:
        res["solo"] = solo_regression(a)
        rel = res["solo"]["parent_spread"] / res["solo"]["parent"]["median"]
    res["local"] = [time_size(N, make_cfg, LOCAL, a.envs, a.frag_len, int(m), -1, a.repeats, rel)
                    for m in a.local.split(",") if m]
    nb = a.frag_len * a.envs * 4 // 128
    res["c4"] = [time_size(N, make_cfg, C4, a.envs, a.frag_len, int(m), nb, a.repeats, rel)
                 for m in a.c4.split(",") if m]
    res["c4_note"] = "C4 updates are capped at one epoch (max_steps = R / 128)"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
