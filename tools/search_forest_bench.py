"""Measure the forest search (oak_amd.search.forest_search on device tensors: one GPU lane per tree, oak_amd/csrc/forest.hip) against
the way to search many positions that existed before it: tree_search_many over the same roots with the same budget and its default
batch, 16 contexts (= 16 host trees) at a time.

Roots: random OU battles built on the device (oakgpu_random_ou_battles_dev), advanced --advance turn-steps of random play; terminal
ones are dropped.  Cells: trees N x budget, for UCB + "fp" (PokeEngine eval), UCB + "mc" and PUCB + net_default; a cell whose arenas
(N x (budget + 1) nodes of 224 bytes + the edge tables) exceed --max-arena-gb is skipped, the baseline runs only up to
--baseline-max-trees, and cells are left out (and listed) once --max-seconds have passed.  Per cell: one warm-up of each form, then
--rounds runs of each, alternated, the order swapped from round to round; times are a host clock around calls that end with the stream
idle.  Reported per cell: the runs, the median, iterations/s (N x budget / s), searches/s, mean levels per tree iteration
(total_depth / iterations), the lockstep levels and kernel launches per iteration, and whether the forest's median beats the
baseline's FASTEST run.

  python tools/search_forest_bench.py [--trees 256,4096,65536] [--budgets 64,256,1024] [--configs ucb_fp,ucb_mc,pucb_default] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"ucb_fp": ("ucb", "poke-engine"), "ucb_mc": ("ucb", "mc"), "pucb_default": ("pucb", "net_default.battle.net")}


def main():
    import torch
    from oak_amd import _lib
    from oak_amd.engine import Context, Network
    from oak_amd.search import Forest, forest_search, tree_search_many
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", default="256,4096,65536")
    ap.add_argument("--budgets", default="64,256,1024")
    ap.add_argument("--configs", default="ucb_fp,ucb_mc,pucb_default")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--advance", type=int, default=6)
    ap.add_argument("--max-arena-gb", type=float, default=48.0)
    ap.add_argument("--baseline-max-trees", type=int, default=4096)
    ap.add_argument("--max-seconds", type=float, default=1e9)
    ap.add_argument("--out")
    a = ap.parse_args()
    t_begin = time.perf_counter()
    torch.cuda.init()   # torch initialises the GPU before the library does
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    ctx.ensure_ou_pools()
    lib, h = ctx.lib, ctx.handle
    P = lambda t: C.c_void_p(t.data_ptr())
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)
    trees, budgets = [int(x) for x in a.trees.split(",")], [int(x) for x in a.budgets.split(",")]
    n_max = max(trees)
    n_gen = n_max + n_max // 4 + 64
    b, d, p, r = u8(n_gen, 384), u8(n_gen, 8), u8(n_gen, 8), u8(n_gen)
    _lib.check(lib.oakgpu_random_ou_battles_dev(h, 0x0A4B00000000, n_gen, P(b), P(d), P(p), P(r)))
    steps, vals = torch.empty(n_gen, dtype=torch.int32, device=dev), torch.empty(n_gen, dtype=torch.float32, device=dev)
    _lib.check(lib.oakgpu_rollout_dev(h, P(b), P(d), P(r), P(p), n_gen, a.advance, 0, P(r), P(steps), P(vals), P(b), P(d)))
    ctx.synchronize()
    live = torch.nonzero((r & 15) == 0).flatten()[:n_max]
    assert live.numel() == n_max, "too few live roots"
    b, d, r = b[live].contiguous(), d[live].contiguous(), r[live].contiguous()
    seeds_np = (np.arange(n_max, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(99)).astype(np.uint64)
    seeds = torch.from_numpy(seeds_np.view(np.int64)).to(dev)
    hb, hd, hr = b.cpu().numpy(), d.cpu().numpy(), r.cpu().numpy()
    ctxs = [Context(0) for _ in range(16)]
    nets = {}

    def evaluator(name):
        if name in ("mc", "poke-engine"):
            return name
        if name not in nets:
            nets[name] = Network(ctx, path=os.path.join(ROOT, "tests", "golden", name))
        return nets[name]

    def forest_run(forest, n, budget, bandit, ev):
        ctx.synchronize()
        t = time.perf_counter()
        out = forest_search(ctx, b[:n], d[:n], r[:n], seeds[:n], budget, c=1.0, bandit=bandit, evaluator=ev, forest=forest)
        ctx.synchronize()
        s = time.perf_counter() - t
        st = forest.last_stats()
        return dict(s=s, iterations_per_s=n * budget / s, searches_per_s=n / s, mean_levels_per_iteration=float(out["total_depth"].sum()) / (n * budget),
                    lockstep_levels_per_iteration=st[1] / budget, launches_per_iteration=st[2] / budget, polls_per_iteration=st[3] / budget,
                    mean_nodes=float(out["nodes"].to(torch.float64).mean()))

    def baseline_run(n, budget, bandit, ev):
        t = time.perf_counter()
        depth = 0
        for s0 in range(0, n, 16):
            k = min(16, n - s0)
            outs = tree_search_many(ctxs[:k], hb[s0:s0 + k], hd[s0:s0 + k], hr[s0:s0 + k], seeds_np[s0:s0 + k], iterations=budget, c=1.0, bandit=bandit, evaluator=ev)
            depth += sum(o["raw"].total_depth for o in outs)
        s = time.perf_counter() - t
        return dict(s=s, iterations_per_s=n * budget / s, searches_per_s=n / s, mean_levels_per_iteration=depth / (n * budget))

    res = {"what": "tools/search_forest_bench.py on one MI355X", "advance": a.advance, "rounds": a.rounds,
           "timing": "host clock around each whole call, the stream idle before and after; one warm-up of each form first",
           "forest": "forest_search on device tensors, a Forest made once per cell (its allocation is not timed)",
           "baseline": "tree_search_many, 16 contexts at a time, default batch (4096), the same roots, seeds and budget",
           "cells": [], "skipped": []}

    def save():
        if a.out:       # (written after every cell: a run cut short keeps what it measured)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    for cfg in a.configs.split(","):
        bandit, ev_name = CONFIGS[cfg]
        ev = evaluator(ev_name)
        for n in trees:
            for budget in budgets:
                slots = 16
                while slots < 2 * (budget + 1):
                    slots *= 2
                gb = n * ((budget + 1) * 224 + slots * 32) / 2 ** 30
                cell = dict(config=cfg, trees=n, budget=budget, arena_gb=gb)
                if gb > a.max_arena_gb:
                    res["skipped"].append(dict(cell, why="arenas above --max-arena-gb"))
                    continue
                if time.perf_counter() - t_begin > a.max_seconds:
                    res["skipped"].append(dict(cell, why="--max-seconds reached"))
                    continue
                forest = Forest(ctx, n, budget, contextual=bandit == "pucb")
                with_base = n <= a.baseline_max_trees
                forest_run(forest, n, min(budget, 16), bandit, ev)
                if with_base:
                    baseline_run(min(n, 32), budget, bandit, ev)
                fr, bl = [], []
                for k in range(a.rounds):
                    for which in (("forest", "baseline") if k % 2 == 0 else ("baseline", "forest")):
                        if which == "forest":
                            fr.append(forest_run(forest, n, budget, bandit, ev))
                        elif with_base:
                            bl.append(baseline_run(n, budget, bandit, ev))
                    print("  %s N=%d budget=%d round %d: forest %.3f s%s" % (cfg, n, budget, k, fr[-1]["s"], ", baseline %.3f s" % bl[-1]["s"] if bl else ""),
                          file=sys.stderr, flush=True)
                forest.close()
                med = float(np.median([x["s"] for x in fr]))
                cell.update(forest_runs=fr, forest_median_s=med, iterations_per_s=n * budget / med, searches_per_s=n / med,
                            mean_levels_per_iteration=fr[0]["mean_levels_per_iteration"], launches_per_iteration=fr[0]["launches_per_iteration"])
                if bl:
                    fastest = min(x["s"] for x in bl)
                    cell.update(baseline_runs=bl, baseline_median_s=float(np.median([x["s"] for x in bl])), baseline_fastest_s=fastest,
                                forest_median_beats_baseline_fastest=bool(med < fastest))
                else:
                    cell["baseline"] = "not run: above --baseline-max-trees"
                res["cells"].append(cell)
                save()
    claim = [c for c in res["cells"] if (c["config"], c["trees"], c["budget"]) == ("pucb_default", 4096, 256) and "baseline_fastest_s" in c]
    res["claim"] = ("at N = 4096, budget 256, PUCB + net_default the forest's median beats the baseline's fastest run: " +
                    (str(claim[0]["forest_median_beats_baseline_fastest"]) if claim else "not measured"))
    save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
