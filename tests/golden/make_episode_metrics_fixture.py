"""Fixture: the episode metrics RLlib 1.0 recorded at the end of the published runs
(Results/**/experiment_state-*.json, checkpoints[0].last_result), one trial per architecture.
Each record is reduced to what tests/test_episode_metrics.py replays through
ddrl_amd.metrics.EpisodeHistory: hist_stats (the 100-episode window: totals, lengths and the
per-policy agent totals), the summary values computed from it, episodes_this_iter and the key
order of last_result.

    python tests/golden/make_episode_metrics_fixture.py     # in the container (needs /root/reference)
"""
import glob
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/Results"
SUMMARY = ("episode_reward_max", "episode_reward_min", "episode_reward_mean", "episode_len_mean",
           "episodes_this_iter", "policy_reward_min", "policy_reward_max", "policy_reward_mean")


def main():
    out = {}
    for f in sorted(glob.glob(os.path.join(REF, "**/experiment_state-*.json"), recursive=True)):
        with open(f) as fh:
            state = json.load(fh)
        ck = state["checkpoints"][0]
        if isinstance(ck, str):
            ck = json.loads(ck)
        last = ck["last_result"]
        arch = last["config"]["env"].replace("QuantrupedMultiEnv_", "")
        if arch in out:
            continue
        rec = {"source": os.path.relpath(f, REF), "env": last["config"]["env"],
               "key_order": [k for k in last if k != "config"],
               "timesteps_total": last["timesteps_total"], "num_healthy_workers": last["num_healthy_workers"],
               "episodes_total": last["episodes_total"], "hist_stats": last["hist_stats"]}
        rec.update({k: last[k] for k in SUMMARY})
        out[arch] = rec
    path = os.path.join(HERE, "episode_metrics.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0)
    print("wrote", path, os.path.getsize(path), "bytes for", sorted(out))


if __name__ == "__main__":
    main()
