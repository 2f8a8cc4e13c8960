"""Measure self-play over the forest search (oak_amd.frames.forest_selfplay: a batch of games resident on the device, one forest search per
turn, oak_amd/csrc/forestplay.hip) against the way to play many games that existed before it: selfplay_games on 16 contexts (16 host-walked
trees at a time) at its default batch and the same budget, over the first --baseline-games of the same games.

Games: the 16 sample teams (tests/golden/ou_sample_teams.json), two drawn per game, seeds from --seed.  Workloads: pucb_default (PUCB +
net_default, c 1.5, mode p0.5-e0.5 for both forms) and ucb_fp (UCB + PokeEngine eval, c 2, mode e), budget --budget.  Every timed run is a
fresh process (this script with --child): it makes its contexts, forest and network, plays a warm-up (the same batch under a length cap of 2
frames: every allocation and kernel load), then times ONE call with a host clock, the stream idle before and after.  Per workload and size:
--rounds forest runs alternated with baseline runs (the baseline's runs are shared by the sizes of a workload); reported: the runs, the
median, games/s and frames/s, the schedule counters, and -- at --nash-size -- one more forest run without the Nash solve, whose difference
to the median is the host Nash solves' share of a call.  The share of the loop's own kernels is a separate rocprofv3 --kernel-trace
--stats run of `--child forest` (see --help of the child arguments), not made here.  --keep-node: the forest runs keep each game's tree
between turns (a kept forest of --keep-arena nodes per tree, 0 = 4 * budget + 1); a run then also reports the keep-node ratio (updates that
found their child / updates), the mean nodes carried into a turn's search, the trees dropped for want of room and the root mismatches; the
cells are named <workload>+keep/<games>.  The baseline is not run with it.

  python tools/forest_selfplay_bench.py [--sizes 256,4096,65536] [--workloads pucb_default,ucb_fp] [--budget 256] [--rounds 3] [--out FILE]
A run that is cut short keeps what it measured: --out is rewritten after every run, and a later run with the same --out goes on from it."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = {"pucb_default": dict(bandit="pucb", c=1.5, eval="net_default.battle.net", mode="p0.5-e0.5"),
             "ucb_fp": dict(bandit="ucb", c=2.0, eval="poke-engine", mode="e")}


def draw(n, seed):
    from policy_match import team_bytes
    pool = team_bytes(os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json"))
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(pool), (n, 2))
    teams = np.concatenate([pool[pick[:, 0]].reshape(n, 30), pool[pick[:, 1]].reshape(n, 30)], axis=1).astype(np.uint8)
    return np.ascontiguousarray(teams), rng.integers(0, 1 << 63, n, dtype=np.uint64), rng.integers(0, 1 << 63, n, dtype=np.uint64)


def child(a):
    from oak_amd.engine import Context, Network
    from oak_amd.frames import forest_selfplay, selfplay_games
    from oak_amd.search import Forest
    w = WORKLOADS[a.workload]
    ctx = Context(0)
    ev = w["eval"] if w["eval"] in ("mc", "poke-engine") else Network(ctx, path=os.path.join(ROOT, "tests", "golden", w["eval"]))
    teams, battle_seeds, seeds = draw(a.games, a.seed)
    if a.child == "forest":
        nash = False if a.no_nash else ("device" if a.device_nash else True)
        forest = Forest(ctx, a.games, a.budget, contextual=w["bandit"] == "pucb", keep_arena=a.keep_arena if a.keep_node else None)
        kw = dict(c=w["c"], bandit=w["bandit"], evaluator=ev, policy_mode=w["mode"], forest=forest, solve_nash=nash, keep_node=a.keep_node)
        forest_selfplay(ctx, teams, battle_seeds, seeds, a.budget, max_battle_length=2, **kw)
        ctx.synchronize()
        stats = {}
        t = time.perf_counter()
        out = forest_selfplay(ctx, teams, battle_seeds, seeds, a.budget, stats=stats, **kw)
        s = time.perf_counter() - t
        frames, kept = int(out[2][out[4] == 0].sum()), int((out[4] == 0).sum())
        res = dict(form="forest", s=s, games=kept, frames=frames, dropped=a.games - kept, bytes=len(out[0]), solve_nash=nash, keep_node=a.keep_node)
        if a.keep_node:
            res.update(keep_node_ratio=stats["nodes_kept"] / max(stats["rows"], 1), mean_kept_nodes_per_turn=stats["carried_nodes"] / max(stats["rows"], 1),
                       trees_dropped=stats.pop("dropped"))
        res.update(stats)
        forest.close()
    else:
        ctxs = [Context(0) for _ in range(16)]
        kw = dict(iterations=a.budget, bandit=w["bandit"], c=w["c"], evaluator=ev, policy_mode=w["mode"])
        selfplay_games(ctxs, teams[:16].reshape(-1, 2, 6, 5), battle_seeds[:16], seeds[:16], max_battle_length=0, **dict(kw, iterations=16))
        t = time.perf_counter()
        frames = 0
        for s0 in range(0, a.games, 16):
            k = min(16, a.games - s0)
            got = selfplay_games(ctxs[:k], teams[s0:s0 + k].reshape(k, 2, 6, 5), battle_seeds[s0:s0 + k], seeds[s0:s0 + k], **kw)
            frames += sum(x[1] for x in got)
        s = time.perf_counter() - t
        res = dict(form="baseline", s=s, games=a.games, frames=frames)
    res.update(games_per_s=res["games"] / s, frames_per_s=res["frames"] / s)
    print("RESULT " + json.dumps(res), flush=True)


def run_child(form, workload, games, budget, seed, no_nash=False, timeout=1100, keep_node=False, keep_arena=0):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", form, "--workload", workload, "--games", str(games), "--budget", str(budget), "--seed", str(seed)]
    if no_nash:
        cmd.append("--no-nash")
    if keep_node:
        cmd += ["--keep-node", "--keep-arena", str(keep_arena)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    lines = [x for x in out.stdout.splitlines() if x.startswith("RESULT ")]
    if out.returncode != 0 or not lines:
        raise RuntimeError("child failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="256,4096,65536")
    ap.add_argument("--workloads", default="pucb_default,ucb_fp")
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-games", type=int, default=256)
    ap.add_argument("--nash-size", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0x0A4B)
    ap.add_argument("--max-seconds", type=float, default=1e9)
    ap.add_argument("--out")
    ap.add_argument("--child", choices=("forest", "baseline"))
    ap.add_argument("--workload", default="ucb_fp")
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--no-nash", action="store_true")
    ap.add_argument("--device-nash", action="store_true", help="child forest: solve the root matrices on the GPU (tools/device_nash_bench.py)")
    ap.add_argument("--keep-node", action="store_true")
    ap.add_argument("--keep-arena", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    t_begin = time.perf_counter()
    res = {"what": "tools/forest_selfplay_bench.py on one MI355X", "budget": a.budget, "rounds": a.rounds,
           "timing": "every run a fresh process; a host clock around one call after a warm-up, the stream idle before and after",
           "forest": "forest_selfplay, host arrays in and the stream copied out, a Forest made before the clock starts",
           "baseline": "selfplay_games, 16 contexts at a time, default batch (1024), the first %d of the same games, the same budget" % a.baseline_games,
           "cells": {}}
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))

    def save():
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    def late():
        return time.perf_counter() - t_begin > a.max_seconds

    sizes = [int(x) for x in a.sizes.split(",")]
    for workload in a.workloads.split(","):
        base = res["cells"].setdefault(workload + "/baseline", {"runs": []})
        for n in sizes:
            cell = res["cells"].setdefault("%s%s/%d" % (workload, "+keep" if a.keep_node else "", n), {"workload": workload, "games": n, "keep_node": a.keep_node, "runs": []})
            for k in range(a.rounds):
                for which in (("forest", "baseline") if k % 2 == 0 else ("baseline", "forest")):
                    if late():
                        continue
                    if which == "forest" and len(cell["runs"]) <= k:
                        cell["runs"].append(run_child("forest", workload, n, a.budget, a.seed, keep_node=a.keep_node, keep_arena=a.keep_arena))
                        print("  %s N=%d forest run %d: %.2f s, %.1f games/s" % (workload, n, k, cell["runs"][-1]["s"], cell["runs"][-1]["games_per_s"]), file=sys.stderr, flush=True)
                    if which == "baseline" and len(base["runs"]) <= k and not a.keep_node:
                        base["runs"].append(run_child("baseline", workload, a.baseline_games, a.budget, a.seed))
                        print("  %s baseline run %d: %.2f s, %.1f games/s" % (workload, k, base["runs"][-1]["s"], base["runs"][-1]["games_per_s"]), file=sys.stderr, flush=True)
                    save()
            if n == a.nash_size and "without_nash" not in cell and cell["runs"] and not late():
                cell["without_nash"] = run_child("forest", workload, n, a.budget, a.seed, no_nash=True, keep_node=a.keep_node, keep_arena=a.keep_arena)
                save()
            if cell["runs"]:
                med = float(np.median([x["s"] for x in cell["runs"]]))
                cell.update(median_s=med, games_per_s=cell["runs"][0]["games"] / med, frames_per_s=cell["runs"][0]["frames"] / med)
                if "without_nash" in cell:
                    cell["host_nash_share_of_a_call"] = 1.0 - cell["without_nash"]["s"] / med
                if base["runs"]:
                    best = max(x["games_per_s"] for x in base["runs"])
                    base.update(median_games_per_s=float(np.median([x["games_per_s"] for x in base["runs"]])), fastest_games_per_s=best)
                    cell["forest_median_beats_baseline_fastest"] = bool(cell["games_per_s"] > best)
            save()
    claim = [res["cells"].get("%s%s/4096" % (w, "+keep" if a.keep_node else ""), {}).get("forest_median_beats_baseline_fastest") for w in a.workloads.split(",")]
    res["claim"] = "at 4,096 games the forest loop's median games/s beats the baseline's fastest run: " + ", ".join(
        "%s: %s" % (w, "not measured" if c is None else c) for w, c in zip(a.workloads.split(","), claim))
    save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
