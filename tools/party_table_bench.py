#!/usr/bin/env python3
"""What the per-search bench-slot table (oakgpu_party_table_*) buys, measured on the GPU -> profiles/r09_party_table.json.

  leaf call : oakgpu_leaf_eval_dev against oakgpu_leaf_eval_table_dev on the same device leaves (descendants of one root, so every
              slot hits), n = 16,384 (the search's batch) and 65,536, on net_default and the 256-wide net;
  search    : oakgpu_search_many over 8 roots, and over one, with the contexts' switch (oakgpu_set_search_party_table) off and on.

Each pair is warmed up, then timed REPEATS times, the two arms alternating inside one process; a sample is a host clock around
CALLS calls that ends in a stream synchronise.  The file keeps every sample, the medians, the spread (min, max) and the ratio
plain / table of the medians.  There is no CPU path: without a GPU the tool fails.
usage: tools/party_table_bench.py [--out FILE] [--repeats N] [--quick]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def summary(samples):
    return {"samples_ms": samples, "median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples)}


def compare(plain, table):
    a, b = summary(plain), summary(table)
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    diff = a["median_ms"] - b["median_ms"]
    return {"plain": a, "table": b, "ratio_plain_over_table": a["median_ms"] / b["median_ms"], "median_gain_ms": diff, "spread_ms": spread,
            "faster_by_more_than_the_spread": bool(diff > spread)}


def leaves_of_one_root(ctx, n, turns, seed):
    """n copies of a random OU root, each advanced `turns` turns on the device with a prng stream of its own -> (battles, durations)
    and results as torch uint8 tensors, and the root's bytes."""
    import torch
    from oak_amd import _lib
    dev = "cuda:%d" % ctx.device
    ctx.ensure_ou_pools()
    rb = torch.zeros((1, 384), dtype=torch.uint8, device=dev)
    rd = torch.zeros((1, 8), dtype=torch.uint8, device=dev)
    rp = torch.zeros((1, 8), dtype=torch.uint8, device=dev)
    rr = torch.zeros(1, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(ctx.lib.oakgpu_random_ou_battles_dev(ctx.handle, int(seed), 1, p(rb), p(rd), p(rp), p(rr)))
    ctx.synchronize()
    b, d = rb.repeat(n, 1).contiguous(), rd.repeat(n, 1).contiguous()
    r = rr.repeat(n).contiguous()
    prng = torch.from_numpy(np.random.default_rng(seed).integers(1, 1 << 63, size=n, dtype=np.uint64).view(np.uint8).reshape(n, 8).copy()).to(dev)
    steps = torch.zeros(n, dtype=torch.int32, device=dev)      # (uint32 on the device; torch's uint32 has few operators)
    vals = torch.zeros(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    for _ in range(turns):
        _lib.check(ctx.lib.oakgpu_rollout_dev(ctx.handle, p(b), p(d), p(r), p(prng), n, 1, 0, p(r), p(steps), p(vals), p(b), p(d)))
    ctx.synchronize()
    return b, d, r, rb.cpu().numpy()[0]


def bench_leaf(ctx, net, n, repeats, calls):
    import torch
    from oak_amd import _lib
    from oak_amd.engine import PartyTable
    dev = "cuda:%d" % ctx.device
    b, d, _, root = leaves_of_one_root(ctx, n, 12, 0xBE7C4 + n)
    table = PartyTable(ctx, net).fill(root)
    emb = torch.zeros((n, net.shape()[0]), dtype=torch.float32, device=dev)
    vp, vt = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    lib, h = ctx.lib, ctx.handle

    def plain():
        _lib.check(lib.oakgpu_leaf_eval_dev(h, net.handle, p(b), p(d), n, p(vp), p(emb)))

    def tabled():
        _lib.check(lib.oakgpu_leaf_eval_table_dev(h, net.handle, table.handle, None, p(b), p(d), n, p(vt), p(emb)))

    def sample(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    for fn in (plain, tabled, plain, tabled):      # warm-up: code objects, workspaces
        sample(fn)
    misses = table.last_misses()
    assert bool((vp == vt).all()), "the table call's values differ from the plain call's"
    sp, st = [], []
    for _ in range(repeats):
        sp.append(sample(plain))
        st.append(sample(tabled))
    out = compare(sp, st)
    out.update(n=n, calls_per_sample=calls, misses=misses, unit="ms per leaf call")
    table.close()
    return out


def bench_search(net, n_roots, repeats, iterations, batch):
    import oak_amd.search as S
    from oak_amd.engine import Context
    ctxs = [Context(0) for _ in range(n_roots)]
    roots = [leaves_of_one_root(ctxs[0], 1, 6, 0x5EA7C0 + k) for k in range(n_roots)]
    battles = np.stack([np.asarray(x[0].cpu().numpy()[0]) for x in roots])
    durations = np.stack([np.asarray(x[1].cpu().numpy()[0]) for x in roots])
    results = np.array([int(x[2].cpu()[0]) for x in roots], dtype=np.uint8)      # (six turns in: no game is over; a terminal root is refused)
    seeds = [100 + k for k in range(n_roots)]

    def run(on):
        for c in ctxs:
            c.set_search_party_table(on)
        t0 = time.perf_counter()
        outs = S.tree_search_many(ctxs, battles, durations, results, seeds, iterations=iterations, batch=batch, bandit="ucb", c=1.5, evaluator=net)
        return (time.perf_counter() - t0) * 1e3, outs

    _, a = run(False)
    _, b = run(True)
    same = all(x["visit_matrix"].tobytes() == y["visit_matrix"].tobytes() and x["value_matrix"].tobytes() == y["value_matrix"].tobytes() for x, y in zip(a, b))
    assert same, "the switch changed a search result"
    sp, st = [], []
    for _ in range(repeats):
        sp.append(run(False)[0])
        st.append(run(True)[0])
    for c in ctxs:
        c.set_search_party_table(False)
        c.close()
    out = compare(sp, st)
    out.update(roots=n_roots, iterations=iterations, batch=batch, unit="ms per oakgpu_search_many call", results_equal=same)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_party_table.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    assert args.repeats >= 5 or args.quick, "at least 5 repeats"
    import torch
    assert torch.cuda.is_available(), "party_table_bench needs a GPU"
    from oak_amd.engine import Context, Network
    ctx = Context(0)
    res = {"what": __doc__.split("\n")[0], "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "leaf": {}, "search": {}}
    sizes = (1024,) if args.quick else (16384, 65536)
    for tag in ("net_default", "net_256"):
        net = Network(ctx, path=os.path.join(GOLDEN, tag + ".battle.net"))
        for n in sizes:
            res["leaf"]["%s_n%d" % (tag, n)] = bench_leaf(ctx, net, n, args.repeats, 4 if args.quick else (200 if n <= 16384 else 60))
            print(tag, n, json.dumps({k: v for k, v in res["leaf"]["%s_n%d" % (tag, n)].items() if k not in ("plain", "table")}), flush=True)
        if tag == "net_default":
            for roots in (8, 1):
                key = "%d_roots" % roots
                res["search"][key] = bench_search(net, roots, args.repeats, 1 << (12 if args.quick else 17), 512 if args.quick else 16384)
                print("search", key, json.dumps({k: v for k, v in res["search"][key].items() if k not in ("plain", "table")}), flush=True)
        net.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
