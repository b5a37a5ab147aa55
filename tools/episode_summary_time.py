"""Host cost of EpisodeHistory.summarize (ddrl_amd/metrics.py) against the per-row implementation
it replaced (tests/episode_summary_reference.py), on synthetic rows: no GPU needed.

    python tools/episode_summary_time.py [--rows 1000,20000,100000] [--repeats 5]

Per row count: milliseconds per call (median of --repeats, a fresh history each, the Local agent
map) of both, and whether the two results are equal.  Prints one JSON line per size.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000,20000,100000")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    from ddrl_amd.metrics import EpisodeHistory
    from tests.episode_summary_reference import EpisodeHistory as Reference
    agent_policy, policy_ids = [0, 1, 2, 3], ["p0", "p1", "p2", "p3"]
    rng = np.random.default_rng(0)
    for n in (int(x) for x in a.rows.split(",")):
        rows = rng.normal(size=(n, 8)) * 50.0
        rows[:, 2] = rng.integers(1, 1001, n)
        ms = {"array": [], "per_row": []}
        for _ in range(a.repeats):
            for name, cls in (("array", EpisodeHistory), ("per_row", Reference)):
                h = cls(100)
                t0 = time.perf_counter()
                out = h.summarize(rows, agent_policy, policy_ids)
                ms[name].append((time.perf_counter() - t0) * 1e3)
                ms[name + "_out"] = out
        same = json.dumps(ms.pop("array_out")) == json.dumps(ms.pop("per_row_out"))
        print(json.dumps({"rows": n, "array_ms": statistics.median(ms["array"]), "per_row_ms": statistics.median(ms["per_row"]),
                          "equal": same}), flush=True)


if __name__ == "__main__":
    main()
