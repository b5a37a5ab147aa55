"""Timing of the group rollout ("Population rollout").

One session, device events around whole calls after a warm-up, three alternating runs of each
variant per size.  One fragment (T steps and the bootstrap) of M members on the device env plane:
  group       one RolloutGroup.run (table copy and T x (6 .. 8) + 1 launches for all members);
  replays     M Context.rollout_devenv calls in stream order (a replayed HIP graph each);
  python      the per-step Python loop PPOTrainer._sample_fragment runs for each member in turn
              (its per-step noise draw included, as the trainer issues it);
  noise       the M x T per-step generator draws into the members' slabs alone -- what a population
              adds in front of `group` (and a caller of `replays` needs too).
Sizes: Local at (M, n) = (1, 4096), (16, 4096), (1, 80), (16, 80) and SharedDecentral at (64, 80),
T = 200.  Per size: milliseconds per call (median, min - max), the ratio replays / group per run,
and whether the group beat the replays in every run by more than the replays' own spread.
  --iterations: whole PopulationTrainer.train() iterations (wall clock, sampling and learning apart)
    at (16, 80) and (16, 4096), group_rollout on and off, alternating.
  --parent-root DIR (a built checkout of the parent commit): the solo ddrl_rollout_devenv fragment
    and bench.py's headline on this tree and on the parent's, child processes, alternating.
  --rng: instead of the above, the device generator ("Device randomness";
    default output profiles/population/rng_time.json).  Whole PopulationTrainer.train() iterations
    with rng_backend "host" and "device", alternating in one process, at the --iterations sizes;
    the fills alone (wall clock around a synchronized call): the two group fills against the host
    draws they replace (M x T torch.randn calls; M x P numpy schedules and their uploads); and, with
    --parent-root, the host backend's iterations on this tree and on the parent's, child processes,
    alternating.
  --finish: instead of the above, the group finish ("Population finish"; default
    output profiles/population/finish_time.json), rng_backend "device" throughout.  At the
    --iterations sizes: PopulationTrainer iterations with group_finish on and off, child processes,
    alternating, each iteration split by synchronizes into chain / finish / learn / learner-statistics
    readback / summary, with the episode rows of every member and iteration; the finish alone at
    M = 1, 4 and 16 (FinishGroup.run against M x (gae + episodes_collect), a fresh fragment in front
    of every call); and, with --parent-root, whole solo PPOTrainer.train() and default
    PopulationTrainer.train() iterations on this tree and on the parent's, child processes, alternating.
Writes one JSON document (default profiles/population/rollout_time.json).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCAL, C4 = "QuantrupedMultiEnv_Local", "QuantrupedMultiEnv_SharedDecentral"


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)   # ms


def make_members(N, make_cfg, env, n_envs, T, M):
    """M contexts with their own weights and device env plane, reset and observed."""
    import numpy as np
    import torch
    from ddrl_amd.trainer import glorot_ffn_flat
    cfg, _ = make_cfg(env, n_envs, T)
    out = []
    for m in range(M):
        ctx = N.Context(cfg, 0, torch.cuda.current_stream().cuda_stream)
        rng = np.random.default_rng(100 + m)
        for p in range(cfg.n_policies):
            ctx.params_set(p, glorot_ffn_flat(rng, cfg.obs_dim[p], cfg.act_dim))
        env_m = N.DevEnv(ctx, seed=7 + m)
        ctx.observe(env_m.reset())
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1000 + m)
        slab = torch.empty((T, n_envs, cfg.n_agents, cfg.act_dim), dtype=torch.float32, device="cuda")
        actions = torch.zeros((n_envs, 8), dtype=torch.float32, device="cuda")
        out.append((ctx, env_m, gen, slab, actions))
    return out, cfg


def time_size(N, make_cfg, env, n_envs, T, M, repeats):
    import torch
    members, cfg = make_members(N, make_cfg, env, n_envs, T, M)
    group = N.RolloutGroup([x[0] for x in members], [x[1] for x in members])
    shape = (n_envs, cfg.n_agents, cfg.act_dim)

    def draws():
        for ctx, env_m, gen, slab, actions in members:
            for t in range(T):
                torch.randn(shape, generator=gen, out=slab[t])

    def run_group():
        group.run([x[3] for x in members])

    def run_replays():
        for ctx, env_m, gen, slab, actions in members:
            ctx.rollout_devenv(env_m, slab)

    def run_python():
        for ctx, env_m, gen, slab, actions in members:
            for t in range(T):
                eps = torch.randn(shape, device="cuda", generator=gen)
                ctx.act(t, eps, actions)
                env_m.step(actions)
                ctx.reward(t, env_m.fw, env_m.cfrc, actions, env_m.done)
                ctx.observe(env_m.obs)
            ctx.bootstrap()
    variants = {"noise": draws, "group": run_group, "replays": run_replays, "python": run_python}
    for fn in variants.values():   # warm-up: code objects, clocks, the graph captures
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(timed(fn))
    group.close()
    for ctx, env_m, *_ in members:
        env_m.close()
        ctx.close()
    spread = max(ms["replays"]) - min(ms["replays"])
    res = {"env": env, "members": M, "envs": n_envs, "frag_len": T, "ms": ms,
           **{f"{k}_ms": summary(v) for k, v in ms.items()},
           "replays_over_group": [b / a for a, b in zip(ms["group"], ms["replays"])],
           "python_over_group": [b / a for a, b in zip(ms["group"], ms["python"])],           "group_us_per_step": statistics.median(ms["group"]) * 1e3 / T,
           "replays_spread_ms": spread,
           "group_beats_replays_every_run_by_more_than_their_spread":
               bool(all(b - a > spread for a, b in zip(ms["group"], ms["replays"])))}
    print(json.dumps({k: v for k, v in res.items() if k != "ms"}), flush=True)
    return res


def time_iterations(M, n_envs, T, repeats):
    """Whole PopulationTrainer.train() iterations, group_rollout on and off, alternating."""
    from ddrl_amd.population import PopulationTrainer
    config = {"env": LOCAL, "env_backend": "device", "rollout_fragment_length": T}
    pops = {name: PopulationTrainer(config, range(M), n_envs=n_envs, group_rollout=on)
            for name, on in (("group_rollout", True), ("member_sampling", False))}
    out = {name: {"iteration_ms": [], "sample_ms": [], "learn_ms": []} for name in pops}
    for it in range(repeats + 1):   # the first iteration of each is the warm-up
        for name, pop in pops.items():
            t0 = time.perf_counter()
            r = pop.train()
            dt = (time.perf_counter() - t0) * 1e3
            if it:
                out[name]["iteration_ms"].append(dt)
                out[name]["sample_ms"].append(r[0]["timers"]["sample_time_ms"])
                out[name]["learn_ms"].append(r[0]["timers"]["learn_time_ms"])
    for pop in pops.values():
        pop.stop()
    res = {"members": M, "envs": n_envs, "frag_len": T,
           **{name: {k: summary(v) for k, v in d.items()} for name, d in out.items()}}
    print(json.dumps(res), flush=True)
    return res


def wall(fn):
    """Milliseconds of fn between two synchronizations: host work and device work."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def time_rng_iterations(M, n_envs, T, repeats, backends=("host", "device")):
    """Whole PopulationTrainer.train() iterations per rng_backend, alternating; the first is the warm-up."""
    from ddrl_amd.population import PopulationTrainer
    config = {"env": LOCAL, "env_backend": "device", "rollout_fragment_length": T}
    pops = {b: PopulationTrainer(config if b == "host" else {**config, "rng_backend": b}, range(M), n_envs=n_envs)
            for b in backends}
    out = {b: {"iteration_ms": [], "sample_ms": [], "learn_ms": []} for b in pops}
    for it in range(repeats + 1):
        for b, pop in pops.items():
            t0 = time.perf_counter()
            r = pop.train()
            dt = (time.perf_counter() - t0) * 1e3
            if it:
                out[b]["iteration_ms"].append(dt)
                out[b]["sample_ms"].append(r[0]["timers"]["sample_time_ms"])
                out[b]["learn_ms"].append(r[0]["timers"]["learn_time_ms"])
    for pop in pops.values():
        pop.stop()
    return {"members": M, "envs": n_envs, "frag_len": T, "runs": out,
            **{b: {k: summary(v) for k, v in d.items()} for b, d in out.items()}}


def rng_verdict(res):
    """device below host by more than the host backend's own spread, per timer."""
    for k in ("iteration_ms", "sample_ms", "learn_ms"):
        h, d = res["runs"]["host"][k], res["runs"]["device"][k]
        spread = max(h) - min(h)
        res[f"{k}_host_spread"] = spread
        res[f"{k}_host_minus_device"] = statistics.median(h) - statistics.median(d)
        res[f"{k}_device_below_host_by_more_than_its_spread"] = bool(res[f"{k}_host_minus_device"] > spread)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}), flush=True)
    return res


def time_rng_fills(N, make_cfg, n_envs, T, M, repeats):
    """The fills alone: the two group launches of the device generator against the host draws of the
    same arrays (what PopulationTrainer issues per iteration with either backend)."""
    import numpy as np
    import torch
    members, cfg = make_members(N, make_cfg, LOCAL, n_envs, T, M)
    ctxs = [x[0] for x in members]
    for m, ctx in enumerate(ctxs):
        ctx.rng_seed(N.RNG_NOISE, 1000 + m)
        ctx.rng_seed(N.RNG_SCHEDULE, 2000 + m)
    slabs = [x[3] for x in members]
    sched = [ctx.schedule_alloc() for ctx in ctxs]
    rngs = [np.random.default_rng(m) for m in range(M)]
    shape = (n_envs, cfg.n_agents, cfg.act_dim)
    R = [T * ctxs[0].layout[p]["C"] for p in range(cfg.n_policies)]
    nb = [max(1, r // cfg.sgd_minibatch_size) for r in R]

    def host_noise():
        for ctx, env_m, gen, slab, actions in members:
            for t in range(T):
                torch.randn(shape, generator=gen, out=slab[t])

    def host_schedule():
        keep = []
        for rng in rngs:
            for p in range(cfg.n_policies):
                sh = rng.permutation(R[p]).astype(np.int32)
                pe = np.stack([rng.permutation(nb[p]) for _ in range(cfg.num_sgd_iter)]).astype(np.int32)
                keep.append((torch.from_numpy(sh).to("cuda"), torch.from_numpy(pe).to("cuda")))

    variants = {"host_noise": host_noise, "noise_fill_group": lambda: N.noise_fill_group(ctxs, T, slabs),
                "host_schedule": host_schedule,
                "schedule_fill_group": lambda: N.schedule_fill_group(ctxs, [s[0] for s in sched], [s[1] for s in sched])}
    for fn in variants.values():
        fn()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(wall(fn))
    for ctx, env_m, *_ in members:
        env_m.close()
        ctx.close()
    res = {"members": M, "envs": n_envs, "frag_len": T, "unit": "milliseconds, wall clock around a synchronized call",
           "runs": ms, **{f"{k}_ms": summary(v) for k, v in ms.items()}}
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}), flush=True)
    return res


def rng_child(root, sizes, T, repeats):
    """Child process: the host backend's iterations on the tree at `root`; one JSON line."""
    sys.path.insert(0, root)
    print(json.dumps([time_rng_iterations(m, n, T, repeats, backends=("host",)) for m, n in sizes]))


def rng_regression(a, sizes):
    trees = (("this", HERE), ("parent", os.path.abspath(a.parent_root)))
    runs = {n: [{k: [] for k in ("iteration_ms", "sample_ms", "learn_ms")} for _ in sizes] for n, _ in trees}
    for rnd in range(a.rounds):
        for name, root in (trees if rnd % 2 == 0 else trees[::-1]):
            got = child_json([sys.executable, os.path.abspath(__file__), "--rng-child", root, "--iterations", a.iterations,
                              "--frag-len", str(a.frag_len), "--repeats", str(a.repeats)], root, f"the rng child of {root}")
            for i, g in enumerate(got):
                for k, v in g["runs"]["host"].items():
                    runs[name][i][k] += v
    out = []
    for i, (m, n) in enumerate(sizes):
        out.append({"members": m, "envs": n,
                    **{k: against({"this": runs["this"][i][k], "parent": runs["parent"][i][k]},
                                  f"{k} of a host-backend PopulationTrainer.train(), Local {m} x {n}; {a.rounds} alternating "
                                  f"processes per tree x {a.repeats}") for k in ("iteration_ms", "sample_ms", "learn_ms")}})
    return out


def main_rng(a):
    sizes = [(int(m), int(n)) for m, n in (s.split(":") for s in a.iterations.split(",") if s)]
    if a.rng_child:
        return rng_child(a.rng_child, sizes, a.frag_len, a.repeats)
    sys.path.insert(0, HERE)
    import torch
    from ddrl_amd import native as N
    from ddrl_amd.spec import make_cfg
    if not torch.cuda.is_available():
        sys.exit("population_rollout_time: needs a GPU (no timing without one)")
    out = a.out or os.path.join(HERE, "profiles", "population", "rng_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit, "frag_len": a.frag_len, "repeats": a.repeats}
    res["iterations"] = [rng_verdict(time_rng_iterations(m, n, a.frag_len, a.repeats)) for m, n in sizes]
    res["fills"] = [time_rng_fills(N, make_cfg, n, a.frag_len, m, a.repeats) for m, n in sizes]
    if a.parent_root:
        res["host_backend_against_parent"] = rng_regression(a, sizes)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


# ---- --finish: the group finish ("Population finish") ----
def split_iteration(pop):
    """One PopulationTrainer.train() with a synchronize between its parts: milliseconds of the rollout
    chain, the finish, the learn launch, the learner-statistics readback and the host-side results
    (update_kl and the episode summary), and the episode rows of every member."""
    import torch
    from ddrl_amd import native as N
    marks = [time.perf_counter()]

    def mark():
        torch.cuda.synchronize()
        marks.append(time.perf_counter())
    if pop.rollout_group is not None:
        pop._sample_group()
    else:
        for t in pop.trainers:
            t._sample_fragment()
    mark()
    pop._finish()
    mark()
    if pop.device_rng:
        N.schedule_fill_group([t.ctx for t in pop.trainers], [t.sched[0] for t in pop.trainers],
                              [t.sched[1] for t in pop.trainers])
    sched = [t._learn_schedules(fill=False) for t in pop.trainers]
    pop.group.run([s[0] for s in sched], [s[1] for s in sched], [t.kl_coeff for t in pop.trainers])
    pop.group.finish()
    mark()
    stats = pop._learn_stats(sched[0][2])
    mark()
    learners = [t._learn_results(s[2], stats[m] if stats else None) for m, (t, s) in enumerate(zip(pop.trainers, sched))]
    results = [t._iteration_result(lr, marks[0], marks[1], marks[3]) for t, lr in zip(pop.trainers, learners)]
    marks.append(time.perf_counter())
    ms = [(b - a) * 1e3 for a, b in zip(marks, marks[1:])]
    return {"chain_ms": ms[0], "finish_ms": ms[1], "learn_ms": ms[2], "stats_readback_ms": ms[3], "summary_ms": ms[4],
            "iteration_ms": sum(ms), "episode_rows": [r["episodes_this_iter"] for r in results]}


def finish_child(root, mode, M, n_envs, T, repeats):
    """Child process on the tree at `root`; one JSON line.  mode: "group" / "members" = the split
    iterations of a population with group_finish on / off (this tree); "population" = whole
    PopulationTrainer.train() calls as the tree ships them; "solo" = whole PPOTrainer.train() calls."""
    sys.path.insert(0, root)
    config = {"env": LOCAL, "env_backend": "device", "rollout_fragment_length": T, "rng_backend": "device"}
    runs = []
    if mode == "solo":
        from ddrl_amd.trainer import PPOTrainer
        tr = PPOTrainer(config, n_envs=n_envs, seed=0)
        for it in range(repeats + 1):
            t0 = time.perf_counter()
            r = tr.train()
            runs.append({"iteration_ms": (time.perf_counter() - t0) * 1e3, "episode_rows": [r["episodes_this_iter"]]})
        tr.stop()
    else:
        from ddrl_amd.population import PopulationTrainer
        kw = {} if mode == "population" else {"group_finish": mode == "group"}
        pop = PopulationTrainer(config, range(M), n_envs=n_envs, **kw)
        for it in range(repeats + 1):
            if mode == "population":
                t0 = time.perf_counter()
                r = pop.train()
                runs.append({"iteration_ms": (time.perf_counter() - t0) * 1e3, "sample_ms": r[0]["timers"]["sample_time_ms"],
                             "learn_ms": r[0]["timers"]["learn_time_ms"], "episode_rows": [x["episodes_this_iter"] for x in r]})
            else:
                runs.append(split_iteration(pop))
        pop.stop()
    print(json.dumps(runs[1:]))   # the first iteration is the warm-up


def finish_children(a, root, mode, M, n):
    return child_json([sys.executable, os.path.abspath(__file__), "--finish-child", root, "--finish-mode", mode,
                       "--members", str(M), "--envs", str(n), "--frag-len", str(a.frag_len), "--repeats", str(a.repeats)],
                      root, f"the {mode} child of {root}")


def columns(runs):
    keys = [k for k in runs[0] if k != "episode_rows"]
    return {**{k: summary([r[k] for r in runs]) for k in keys}, "runs": runs}


def time_finish_alone(N, make_cfg, n_envs, T, M, repeats):
    """The finish alone: FinishGroup.run (rows included) against M x (gae + episodes_collect), wall
    clock around a synchronized call, a fresh device-plane fragment in front of every call."""
    members, cfg = make_members(N, make_cfg, LOCAL, n_envs, T, M)
    ctxs = [x[0] for x in members]
    group = N.FinishGroup(ctxs)
    rows = []

    def fragment():
        for ctx, env_m, gen, slab, actions in members:
            slab.normal_(generator=gen)
            ctx.rollout_devenv(env_m, slab)

    def run_group():
        rows.append([int(r.shape[0]) for r in group.run()])

    def run_members():
        for ctx in ctxs:
            ctx.gae()
            ctx.episodes_collect()
    variants = {"group": run_group, "members": run_members}
    ms = {k: [] for k in variants}
    for it in range(repeats + 1):   # the first round is the warm-up
        for k, fn in variants.items():
            fragment()
            dt = wall(fn)
            if it:
                ms[k].append(dt)
    group.close()
    for ctx, env_m, *_ in members:
        env_m.close()
        ctx.close()
    spread = max(ms["members"]) - min(ms["members"])
    res = {"members": M, "envs": n_envs, "frag_len": T, "unit": "milliseconds, wall clock around a synchronized call",
           "runs": ms, **{f"{k}_ms": summary(v) for k, v in ms.items()},
           "members_over_group": statistics.median(ms["members"]) / statistics.median(ms["group"]),
           "members_spread_ms": spread, "episode_rows_per_member": rows,
           "group_beats_members_every_run_by_more_than_their_spread":
               bool(all(b - a > spread for a, b in zip(ms["group"], ms["members"])))}
    print(json.dumps({k: v for k, v in res.items() if k not in ("runs", "episode_rows_per_member")}), flush=True)
    return res


def main_finish(a):
    if a.finish_child:
        return finish_child(a.finish_child, a.finish_mode, a.members, a.envs, a.frag_len, a.repeats)
    sys.path.insert(0, HERE)
    import torch
    from ddrl_amd import native as N
    from ddrl_amd.spec import make_cfg
    if not torch.cuda.is_available():
        sys.exit("population_rollout_time: needs a GPU (no timing without one)")
    out = a.out or os.path.join(HERE, "profiles", "population", "finish_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    sizes = [(int(m), int(n)) for m, n in (s.split(":") for s in a.iterations.split(",") if s)]
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit, "frag_len": a.frag_len, "repeats": a.repeats,
           "rounds": a.rounds, "iterations": [], "finish_alone": []}

    def dump():   # after every section: a run that is cut short leaves what it has measured
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    for M, n in sizes:
        runs = {"group": [], "members": []}
        for rnd in range(a.rounds):   # neither variant always follows the other
            for mode in (("group", "members") if rnd % 2 == 0 else ("members", "group")):
                runs[mode] += finish_children(a, HERE, mode, M, n)
        entry = {"members": M, "envs": n, "frag_len": a.frag_len, **{k: columns(v) for k, v in runs.items()}}
        fm = [r["finish_ms"] for r in runs["members"]]
        spread = max(fm) - min(fm)
        gain = statistics.median(fm) - statistics.median([r["finish_ms"] for r in runs["group"]])
        entry.update({"finish_members_spread_ms": spread, "finish_members_minus_group_ms": gain,
                      "group_finish_faster_by_more_than_the_members_spread": bool(gain > spread),
                      "episode_rows_per_member_and_iteration": [r["episode_rows"] for r in runs["group"]]})
        print(json.dumps({k: v for k, v in entry.items() if k not in ("group", "members", "episode_rows_per_member_and_iteration")}
                         | {m: {k: v for k, v in entry[m].items() if k != "runs"} for m in ("group", "members")}), flush=True)
        res["iterations"].append(entry)
        for alone_m in (1, 4, 16):
            res["finish_alone"].append(time_finish_alone(N, make_cfg, n, a.frag_len, alone_m, a.repeats))
        dump()
    if a.parent_root:
        trees = (("this", HERE), ("parent", os.path.abspath(a.parent_root)))
        res["against_parent"] = []
        for M, n in sizes:
            for mode in ("solo", "population"):
                it = {"this": [], "parent": []}
                rows = {"this": [], "parent": []}
                for rnd in range(a.rounds):
                    for name, root in (trees if rnd % 2 == 0 else trees[::-1]):
                        got = finish_children(a, root, mode, M, n)
                        it[name] += [r["iteration_ms"] for r in got]
                        rows[name] += [r["episode_rows"] for r in got]
                what = "PPOTrainer.train()" if mode == "solo" else f"PopulationTrainer.train() of {M} seeds, defaults"
                res["against_parent"].append({"mode": mode, "members": 1 if mode == "solo" else M, "envs": n, "episode_rows": rows,
                                              **against(it, f"milliseconds per {what}, Local, {n} envs x {a.frag_len} steps, "
                                                            f"rng_backend device; {a.rounds} alternating processes per tree x {a.repeats}")})
                dump()
    dump()


def solo_child(root, n_envs, T, repeats):
    """Child process: the solo ddrl_rollout_devenv fragment of Local on the tree at `root`; one JSON line."""
    sys.path.insert(0, root)
    import torch
    from ddrl_amd import native as N
    from ddrl_amd.spec import make_cfg
    members, cfg = make_members(N, make_cfg, LOCAL, n_envs, T, 1)
    ctx, env_m, gen, slab, actions = members[0]
    slab.normal_(generator=gen)
    run = lambda: ctx.rollout_devenv(env_m, slab)
    run()
    torch.cuda.synchronize()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "ms": [timed(run) for _ in range(repeats)]}))


def child_json(cmd, cwd, what):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f"population_rollout_time: {what} failed:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def against(out, unit):
    res = {"unit": unit, "this": summary(out["this"]), "parent": summary(out["parent"]), "runs": out}
    res["parent_spread"] = res["parent"]["max"] - res["parent"]["min"]
    res["this_minus_parent"] = res["this"]["median"] - res["parent"]["median"]
    res["within_parent_spread"] = bool(abs(res["this_minus_parent"]) <= res["parent_spread"])
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}), flush=True)
    return res


def solo_regression(a):
    trees = (("this", HERE), ("parent", os.path.abspath(a.parent_root)))
    frag = {"this": [], "parent": []}
    bench = {"this": [], "parent": []}
    for rnd in range(a.rounds):
        for name, root in (trees if rnd % 2 == 0 else trees[::-1]):   # neither tree always follows the other
            frag[name] += child_json([sys.executable, os.path.abspath(__file__), "--solo-child", root, "--envs", str(a.envs),
                                      "--frag-len", str(a.frag_len), "--repeats", str(a.repeats)], root,
                                     f"the solo child of {root}")["ms"]
            bench[name].append(child_json([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3",
                                           "--warmup", "1"], root, f"bench.py of {root}")["value"])
    return {"fragment": against(frag, f"milliseconds per solo ddrl_rollout_devenv fragment, Local, {a.envs} envs x "
                                      f"{a.frag_len} steps; {a.rounds} alternating processes per tree x {a.repeats}"),
            "bench": against(bench, f"bench.py --gpus 1 --steps 3 --warmup 1 headline (env-steps/s); {a.rounds} "
                                    "alternating processes per tree")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096, help="the large size (the small one is 80)")
    ap.add_argument("--frag-len", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="--parent-root: processes per tree")
    ap.add_argument("--sizes", default="local:1:4096,local:16:4096,local:1:80,local:16:80,c4:64:80",
                    help="env:members:envs, comma separated ('' skips the fragment timing)")
    ap.add_argument("--iterations", default="16:80,16:4096", help="members:envs of the whole-iteration timing ('' skips it)")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit (the solo regression)")
    ap.add_argument("--solo-child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--rng", action="store_true", help="time the device generator (rng_backend host against device)")
    ap.add_argument("--rng-child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--finish", action="store_true", help="time the group finish (group_finish on against off)")
    ap.add_argument("--finish-child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--finish-mode", default="group", help=argparse.SUPPRESS)
    ap.add_argument("--members", type=int, default=16, help=argparse.SUPPRESS)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default="", help="default: profiles/population/rollout_time.json (rng_time.json with --rng, "
                                              "finish_time.json with --finish)")
    a = ap.parse_args()
    if a.solo_child:
        return solo_child(a.solo_child, a.envs, a.frag_len, a.repeats)
    if a.finish or a.finish_child:
        return main_finish(a)
    if a.rng or a.rng_child:
        return main_rng(a)
    a.out = a.out or os.path.join(HERE, "profiles", "population", "rollout_time.json")
    sys.path.insert(0, HERE)
    import torch
    from ddrl_amd import native as N
    from ddrl_amd.spec import make_cfg
    if not torch.cuda.is_available():
        sys.exit("population_rollout_time: needs a GPU (no timing without one)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit, "frag_len": a.frag_len, "repeats": a.repeats}
    if a.parent_root:
        res["solo"] = solo_regression(a)
    envs = {"local": LOCAL, "c4": C4}
    res["fragment"] = [time_size(N, make_cfg, envs[e], int(n), a.frag_len, int(m), a.repeats)
                       for e, m, n in (s.split(":") for s in a.sizes.split(",") if s)]
    res["iterations"] = [time_iterations(int(m), int(n), a.frag_len, a.repeats)
                         for m, n in (s.split(":") for s in a.iterations.split(",") if s)]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
