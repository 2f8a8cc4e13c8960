"""Measure the exact Nash solve on the device (oak_amd/csrc/nashdev.hip) against the host solve it replaces in the forest loops.

Solver alone.  The root payoffs of one UCB + PokeEngine forest search over --sizes trees at --budget (openings of games drawn as
tools/forest_selfplay_bench.py draws them) are written to a file; then, alternated, --rounds device runs and --rounds host runs, every run
a fresh process.  A device run times oakgpu_nash_solve_dev over the resident rows with a host clock, the stream idle before and after, after
one warm-up call.  A host run times the other build's oakgpu_solve_matrix over the same rows on 16 threads, the rows split as the loops'
solve_rows splits them -- that solver, its threads and its split, called through ctypes (which drops the GIL) because solve_rows itself
has no entry point; --parent DIR names the build whose solver is timed (a checkout of the parent commit, built), and the same run on this
build shows what the shared solver text's new exact division does on the host.  Reported: seconds and matrices/s per run, medians, and
whether the device's median time at the largest size is below the host's fastest run.

In the loop.  forest_selfplay at --loop-games games, the workloads of tools/forest_selfplay_bench.py, three variants alternated, every run
that tool's `--child forest` in a fresh process: solve_nash 1 on the parent build, 1 on this build, 2 on this build.  Reported: the runs,
medians, whether this build's unchanged path lies within the spread of the parent's runs, the device path against the parent's fastest run,
and the calls' host traffic (loop_syncs, loop_copies, host_reads).

Kernel resources: k_nash_solve<4> and <8> from profiles/<tag>_kernel_resources.json (tools/kernel_resources.py <tag>) when it is there.

  python tools/device_nash_bench.py --parent DIR [--sizes 4096,65536] [--budget 256] [--rounds 3] [--loop-games 4096]
         [--workloads ucb_fp,pucb_default] [--max-seconds S] [--tag r23] [--out profiles/r23_device_nash.json]
A run that is cut short keeps what it measured: --out is rewritten after every run."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_payoffs(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from forest_selfplay_bench import draw
    from oak_amd import _lib
    from oak_amd.engine import Context
    from oak_amd.search import Forest
    ctx = Context(0)
    n = a.trees
    teams, battle_seeds, seeds = draw(n, a.seed)
    b, d, r = ctx.battle(teams, battle_seeds)
    forest = Forest(ctx, n, a.budget)
    prm = _lib.SearchParams(iterations=a.budget, batch=1, ucb_c=2.0, bandit=0, eval=2, max_depth=0, root_rolls=3, other_rolls=1, seed=0, matrix_ucb=0,
                            mucb_delay=0, mucb_minimum=0, mucb_c=0.0, exp3_alpha=-1.0, duration_us=0)
    outs = (_lib.SearchOutput * n)()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    b, d, r, seeds = (np.ascontiguousarray(x) for x in (b, d, r, seeds))
    t = time.perf_counter()
    _lib.check(ctx.lib.oakgpu_forest_search(forest.handle, None, C.byref(prm), vp(b), vp(d), vp(r), vp(seeds), n, outs, 0, None, None, 0))
    search_s = time.perf_counter() - t
    raw = np.frombuffer(outs, dtype=np.uint8).reshape(n, C.sizeof(_lib.SearchOutput))
    at = lambda f: getattr(_lib.SearchOutput, f).offset
    m, nn = raw[:, at("m")].astype(np.int64), raw[:, at("n")].astype(np.int64)
    vis = raw[:, at("visit_matrix"):at("visit_matrix") + 648].copy().view(np.uint64).reshape(n, 9, 9)
    val = raw[:, at("value_matrix"):at("value_matrix") + 648].copy().view(np.float64).reshape(n, 9, 9)
    pay = (val / np.maximum(vis, 1).astype(np.float64) * 256.0).astype(np.int32)       # the loops' payoff kernel: value / visits * 256, truncated
    rows = np.zeros((n, 82), np.int32)
    for g in range(n):
        rows[g, :m[g] * nn[g]] = pay[g, :m[g], :nn[g]].reshape(-1)
    rows[:, 81] = m | nn << 8
    np.save(a.rows, rows)
    forest.close()
    print("RESULT " + json.dumps(dict(trees=n, search_s=search_s, mean_m=float(m.mean()), mean_n=float(nn.mean()), largest_entry=int(rows[:, :81].max()))), flush=True)


def child_device(a):
    sys.path.insert(0, ROOT)
    from oak_amd import _lib
    from oak_amd.engine import Context
    rows = np.load(a.rows)
    n = len(rows)
    ctx = Context(0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    d_pay, d_out = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_pay), rows.nbytes) == 0 and hip.hipMalloc(C.byref(d_out), n * 19 * 8) == 0
    assert hip.hipMemcpy(d_pay, rows.ctypes.data_as(C.c_void_p), rows.nbytes, 1) == 0
    _lib.check(ctx.lib.oakgpu_nash_solve_dev(ctx.handle, d_pay, n, d_out))
    ctx.synchronize()
    t = time.perf_counter()
    _lib.check(ctx.lib.oakgpu_nash_solve_dev(ctx.handle, d_pay, n, d_out))
    ctx.synchronize()
    s = time.perf_counter() - t
    out = np.zeros(n * 19)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d_out, out.nbytes, 2) == 0
    print("RESULT " + json.dumps(dict(form="device", matrices=n, s=s, matrices_per_s=n / s, checksum=float(out[n * 18:].sum()))), flush=True)


def child_host(a):
    root = os.path.abspath(a.lib_root)
    sys.path.insert(0, root)
    from oak_amd import _lib
    lib = _lib.load()
    rows = np.load(a.rows)
    n = len(rows)
    out = np.zeros(n * 19)
    fn = lib.oakgpu_solve_matrix
    base, p1, p2, v = rows.ctypes.data, out.ctypes.data, out.ctypes.data + n * 72, out.ctypes.data + n * 144
    shapes = [(int(x) & 0xFF, (int(x) >> 8) & 0xFF) for x in rows[:, 81]]
    threads = min(16, n // 32 + 1)           # solve_rows' rule on a machine with 16 usable cores
    per = (n + threads - 1) // threads

    def work(lo, hi):
        for g in range(lo, hi):
            m, k = shapes[g]
            if 1 <= m <= 9 and 1 <= k <= 9:
                fn(base + g * 328, m, k, 256, p1 + g * 72, p2 + g * 72, v + g * 8)

    def run():
        pool = [threading.Thread(target=work, args=(min(n, t * per), min(n, (t + 1) * per))) for t in range(threads)]
        t0 = time.perf_counter()
        for th in pool:
            th.start()
        for th in pool:
            th.join()
        return time.perf_counter() - t0

    work(0, min(n, 64))
    s = run()
    print("RESULT " + json.dumps(dict(form="host", build=a.label, threads=threads, matrices=n, s=s, matrices_per_s=n / s, checksum=float(out[n * 18:].sum()))), flush=True)


def run(cmd, timeout=1100):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    lines = [x for x in out.stdout.splitlines() if x.startswith("RESULT ")]
    if out.returncode != 0 or not lines:
        raise RuntimeError("child failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
    return json.loads(lines[-1][7:])


def median(runs, key="s"):
    return float(np.median([x[key] for x in runs]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="a built checkout of the parent commit (its oak_amd and tools are used for the host runs)")
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-games", type=int, default=4096)
    ap.add_argument("--workloads", default="ucb_fp,pucb_default")
    ap.add_argument("--seed", type=int, default=0x0A4B)
    ap.add_argument("--max-seconds", type=float, default=1e9)
    ap.add_argument("--tag", default="r23")
    ap.add_argument("--out")
    ap.add_argument("--child", choices=("payoffs", "device", "host"))
    ap.add_argument("--trees", type=int, default=4096)
    ap.add_argument("--rows")
    ap.add_argument("--lib-root", default=ROOT)
    ap.add_argument("--label", default="this")
    a = ap.parse_args()
    if a.child:
        return {"payoffs": child_payoffs, "device": child_device, "host": child_host}[a.child](a)
    t_begin = time.perf_counter()
    late = lambda: time.perf_counter() - t_begin > a.max_seconds
    me = [sys.executable, os.path.abspath(__file__)]
    res = {"what": "tools/device_nash_bench.py on one MI355X", "budget": a.budget, "rounds": a.rounds,
           "timing": "every run a fresh process; a host clock around one call after a warm-up, the stream idle before and after",
           "host": "oakgpu_solve_matrix of the named build over the same rows on min(16, rows / 32 + 1) threads, the rows split as solve_rows splits them, called through ctypes",
           "solver": {}, "loop": {}}
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))

    def save():
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    builds = [("this", ROOT)] + ([("parent", os.path.abspath(a.parent))] if a.parent else [])
    with tempfile.TemporaryDirectory() as td:
        for n in [int(x) for x in a.sizes.split(",") if x]:
            cell = res["solver"].setdefault(str(n), {"device": [], "host_this": [], "host_parent": []})
            rows = os.path.join(td, "rows%d.npy" % n)
            if late():
                continue
            cell["input"] = run(me + ["--child", "payoffs", "--trees", str(n), "--budget", str(a.budget), "--seed", str(a.seed), "--rows", rows])
            for k in range(a.rounds):
                order = ["device"] + ["host_" + name for name, _ in builds]
                for which in (order if k % 2 == 0 else order[::-1]):
                    if late() or len(cell[which]) > k:
                        continue
                    if which == "device":
                        cell[which].append(run(me + ["--child", "device", "--rows", rows]))
                    else:
                        name = which[5:]
                        cell[which].append(run(me + ["--child", "host", "--rows", rows, "--lib-root", dict(builds)[name], "--label", name]))
                    print("  solver N=%d %s run %d: %.4f s" % (n, which, k, cell[which][-1]["s"]), file=sys.stderr, flush=True)
                    save()
            for which in ("device", "host_this", "host_parent"):
                if cell[which]:
                    cell[which + "_median_s"] = median(cell[which])
                    cell[which + "_median_matrices_per_s"] = n / cell[which + "_median_s"]
            if cell["device"] and cell["host_parent"]:
                cell["host_parent_fastest_s"] = min(x["s"] for x in cell["host_parent"])
                cell["device_median_below_host_parent_fastest"] = bool(cell["device_median_s"] < cell["host_parent_fastest_s"])
                assert all(abs(x["checksum"] - cell["host_parent"][0]["checksum"]) == 0 for x in cell["device"] + cell["host_this"]), "the runs disagree on the values"
            save()
    variants = ([("parent_host", os.path.abspath(a.parent), [])] if a.parent else []) + [("this_host", ROOT, []), ("this_device", ROOT, ["--device-nash"])]
    for workload in [w for w in a.workloads.split(",") if w]:
        cell = res["loop"].setdefault("%s/%d" % (workload, a.loop_games), {name: [] for name, _, _ in variants})
        for k in range(a.rounds):
            for name, root, extra in (variants if k % 2 == 0 else variants[::-1]):
                if late() or len(cell.setdefault(name, [])) > k:
                    continue
                cell[name].append(run([sys.executable, os.path.join(root, "tools", "forest_selfplay_bench.py"), "--child", "forest", "--workload", workload,
                                       "--games", str(a.loop_games), "--budget", str(a.budget), "--seed", str(a.seed)] + extra))
                print("  loop %s %s run %d: %.2f s" % (workload, name, k, cell[name][-1]["s"]), file=sys.stderr, flush=True)
                save()
        for name, _, _ in variants:
            if cell.get(name):
                cell[name + "_median_s"] = median(cell[name])
        if cell.get("parent_host") and cell.get("this_host"):
            lo, hi = min(x["s"] for x in cell["parent_host"]), max(x["s"] for x in cell["parent_host"])
            cell["parent_host_spread_s"] = [lo, hi]
            cell["this_host_median_within_parent_spread"] = bool(lo <= cell["this_host_median_s"] <= hi)
            if cell.get("this_device"):
                cell["this_device_median_over_parent_fastest"] = cell["this_device_median_s"] / lo
                assert all(x["frames"] == cell["parent_host"][0]["frames"] and x["bytes"] == cell["parent_host"][0]["bytes"] for x in cell["this_host"] + cell["this_device"]), \
                    "the variants played other games"
        save()
    path = os.path.join(ROOT, "profiles", "%s_kernel_resources.json" % a.tag)
    if os.path.exists(path):
        kernels = {}
        for name, k in json.load(open(path)).items():
            if "k_nash_solve" in name:
                granule = -(-k["vgpr_count"] // 8) * 8
                kernels["k_nash_solve<%s>" % name.split("<")[1][0]] = dict(vgprs=k["vgpr_count"], sgprs=k["sgpr_count"], lds_bytes=k["group_segment_fixed_size"],
                                                                          scratch_bytes=k["private_segment_fixed_size"], vgpr_spills=k["vgpr_spill_count"],
                                                                          waves_per_simd=min(8, 512 // granule), workgroup=k["max_flat_workgroup_size"])
        res["kernel_resources"] = kernels
    save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
