"""Measure what fast searches (generate's --fast-budget / --fast-search-prob; oakgpu_selfplay_params) buy the device game loop
(oak_amd.frames.forest_selfplay): the same games with fast search off and with --fast-budget at --fast-search-prob, and one control run with
the turn's two-class partition switched off (oakgpu_forest_selfplay_set_partition(0), a benchmark-only switch for one call: the rows stay in game order, so
finished trees stay inside the launches' row ranges and launched exceeds run).

Per workload of tools/forest_selfplay_bench.py (pucb_default: PUCB + net_default; ucb_fp: UCB + PokeEngine), in ONE process: a forest made
once, a warm-up (the batch under a length cap of 2 frames, both modes), then --rounds rounds that alternate the two modes, each run ONE
call timed with a host clock, the stream idle before and after; then the control run.  Recorded per mode: the runs, the median seconds,
games/s, frames/s, full frames/s (the frames training keeps with --min-iterations = fast_budget + 1) and the launched and run tree-iterations;
per workload the measured time ratio fast / off beside the ratio of run tree-iterations, which is what the counters predict.  The games of
the two modes are not the same games (the fast draw shifts every stream), so the ratios compare two samples of the same distribution.

  python tools/fast_search_bench.py [--games 4096] [--budget 256] [--fast-budget 64] [--fast-search-prob 0.75] [--rounds 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    from forest_selfplay_bench import WORKLOADS, draw
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--fast-budget", type=int, default=64)
    ap.add_argument("--fast-search-prob", type=float, default=0.75)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", default="pucb_default,ucb_fp")
    ap.add_argument("--seed", type=int, default=0x0A4B)
    ap.add_argument("--out")
    a = ap.parse_args()
    from oak_amd import _lib
    from oak_amd.engine import Context, Network
    from oak_amd.frames import forest_selfplay
    from oak_amd.search import Forest
    res = {"what": "tools/fast_search_bench.py on one MI355X", "games": a.games, "budget": a.budget, "fast_budget": a.fast_budget,
           "fast_search_prob": a.fast_search_prob, "rounds": a.rounds, "solve_nash": "device",
           "timing": "one process per workload; a host clock around one forest_selfplay call after a warm-up, the stream idle before and after; the modes alternate",
           "workloads": {}}
    ctx = Context(0)
    teams, battle_seeds, seeds = draw(a.games, a.seed)
    modes = {"off": dict(), "fast": dict(fast_budget=a.fast_budget, fast_search_prob=a.fast_search_prob)}
    for name in a.workloads.split(","):
        w = WORKLOADS[name]
        ev = w["eval"] if w["eval"] in ("mc", "poke-engine") else Network(ctx, path=os.path.join(ROOT, "tests", "golden", w["eval"]))
        forest = Forest(ctx, a.games, max(a.budget, a.fast_budget), contextual=w["bandit"] == "pucb")
        kw = dict(c=w["c"], bandit=w["bandit"], evaluator=ev, policy_mode=w["mode"], forest=forest, solve_nash="device")

        def run(mode):
            ctx.synchronize()
            stats = {}
            t = time.perf_counter()
            out = forest_selfplay(ctx, teams, battle_seeds, seeds, a.budget, stats=stats, **kw, **modes[mode])
            s = time.perf_counter() - t
            kept = out[4] == 0
            r = dict(s=s, games=int(kept.sum()), frames=int(out[2][kept].sum()), fast_frames=stats["fast_frames"], full_frames=stats["full_frames"],
                     launched=stats["launched"], run=stats["run"], turns=stats["turns"], rows=stats["rows"])
            print("  %s %s: %.2f s, %d frames (%d full), launched %d, run %d" % (name, mode, s, r["frames"], r["full_frames"], r["launched"], r["run"]), file=sys.stderr, flush=True)
            return r

        for mode in modes:
            forest_selfplay(ctx, teams, battle_seeds, seeds, a.budget, max_battle_length=2, **kw, **modes[mode])
        cell = {mode: {"runs": []} for mode in modes}
        for k in range(a.rounds):
            for mode in (("off", "fast") if k % 2 == 0 else ("fast", "off")):
                cell[mode]["runs"].append(run(mode))
        _lib.check(ctx.lib.oakgpu_forest_selfplay_set_partition(forest.handle, 0))   # (holds for the next call only)
        cell["fast_without_partition"] = {"runs": [run("fast")]}
        for c in cell.values():
            runs = c["runs"]
            med = float(np.median([x["s"] for x in runs]))
            mid = sorted(runs, key=lambda x: x["s"])[len(runs) // 2]
            c.update(median_s=med, games_per_s=mid["games"] / med, frames_per_s=mid["frames"] / med, full_frames_per_s=mid["full_frames"] / med,
                     launched=mid["launched"], run=mid["run"])
        cell["time_ratio_fast_over_off"] = cell["fast"]["median_s"] / cell["off"]["median_s"]
        cell["run_ratio_fast_over_off"] = cell["fast"]["run"] / cell["off"]["run"]
        cell["full_frames_per_s_ratio_fast_over_off"] = cell["fast"]["full_frames_per_s"] / cell["off"]["full_frames_per_s"]
        cell["time_ratio_without_partition_over_fast"] = cell["fast_without_partition"]["median_s"] / cell["fast"]["median_s"]
        res["workloads"][name] = cell
        forest.close()
        if not isinstance(ev, str):
            ev.close()
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    ctx.close()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
