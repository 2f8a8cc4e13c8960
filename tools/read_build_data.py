#!/usr/bin/env python3
"""Read `.build.data` files back on the GPU (oak_amd.build.TrajectoryCorpus): the count of records per status, and histograms of start, end
and the lengths of the legal lists.

usage: tools/read_build_data.py DIR_OR_FILE...            the census of every record
       tools/read_build_data.py --bench [--out FILE]      the time per decode call -> profiles/r28_build_traj.json

--bench needs no files: it decodes a corpus of seeded rollouts (tests/build_traj_ref.py's).  Per size (4,096 and 65,536 rows), mask dtype
(int64, int16) and with / without the mask it takes the median of three timings (each over 16 or 2 calls back to back) of the sample call, alternated in one process with a
torch.full(..., -1) of the same mask tensor on the same device -- a measured fill floor for a store-bound kernel, not a datasheet figure --
and records the implied GB/s of both (the bytes a call must write over its time).  A host clock around work that ends in a device
synchronise.  Without a GPU it fails: there is no CPU decode to time."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def census(ctx, paths):
    from oak_amd import build
    with build.TrajectoryCorpus(ctx, paths) as corpus:
        info = corpus.info()
        start, end, lengths = np.zeros(32, np.int64), np.zeros(32, np.int64), np.zeros(build.MAX_ACTIONS + 1, np.int64)
        for lo in range(0, corpus.records, 16384):
            got = corpus.decode(np.arange(lo, min(lo + 16384, corpus.records), dtype=np.uint32), mask=False)
            ok = got["status"] == 0
            start += np.bincount(got["start"][ok], minlength=32)
            end += np.bincount(got["end"][ok], minlength=32)
            read = np.arange(31)[None, :]
            read = ok[:, None] & (read >= got["start"][:, None]) & (read < got["end"][:, None])
            lengths += np.bincount(got["n_legal"][read], minlength=build.MAX_ACTIONS + 1)
    print("%d records in %d files" % (info["records"], info["files"]))
    for name, count in info["status"].items():
        print("  %-14s %d" % (name, count))
    for name, hist in (("start", start), ("end", end)):
        print(name + ": " + " ".join("%d:%d" % (k, c) for k, c in enumerate(hist) if c))
    edges = (1, 2, 3, 5, 9, 17, 33, 65, 129, 257, build.MAX_ACTIONS + 1)
    print("list lengths: " + " ".join("%d-%d:%d" % (a, b - 1, lengths[a:b].sum()) for a, b in zip(edges, edges[1:]) if lengths[a:b].sum()))


def bench(ctx, out_path):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import build_traj_ref as T
    from oak_amd import build
    records = T.rollout_records(2000, 28)
    result = {"corpus_records": len(records), "runs_per_figure": 3, "cases": []}
    with build.TrajectoryCorpus(ctx, records.tobytes()) as corpus:
        for n in (4096, 65536):
            for dtype, tdt, size in (("int64", torch.int64, 8), ("int16", torch.int16, 2)):
                for mask in (True, False):
                    tensor = torch.empty((n, 31, 339), dtype=tdt, device="cuda")
                    out = {"mask": tensor} if mask else {}
                    for name, shape, dt in (("action", (n, 31), torch.int64), ("n_legal", (n, 31), torch.int16), ("policy", (n, 31), torch.float32),
                                            ("value", (n,), torch.float32), ("score", (n,), torch.float32), ("start", (n,), torch.int64),
                                            ("end", (n,), torch.int64), ("status", (n,), torch.uint8), ("t_max", (1,), torch.int32)):
                        out[name] = torch.empty(shape, dtype=dt, device="cuda")
                    small = sum(v.numel() * v.element_size() for k, v in out.items() if k != "mask") + 4 * n
                    written = small + (tensor.numel() * size if mask else 0)

                    def decode():
                        corpus.sample(n, 1, mask_dtype=dtype, mask=mask, device="cuda", out=dict(out))

                    def fill():
                        tensor.fill_(-1)
                    times, reps = {"decode": [], "fill": []}, (16 if n == 4096 else 2)     # calls per timing: a window of milliseconds at least
                    for f in (decode, fill):
                        f()
                    torch.cuda.synchronize()
                    for _ in range(3):
                        for name, f in (("decode", decode), ("fill", fill)):
                            t0 = time.perf_counter()
                            for _ in range(reps):
                                f()
                            torch.cuda.synchronize()
                            times[name].append((time.perf_counter() - t0) / reps)
                    d, f = float(np.median(times["decode"])), float(np.median(times["fill"]))
                    case = {"rows": n, "mask_dtype": dtype, "mask": mask, "decode_ms": d * 1e3, "decode_gb_s": written / d / 1e9, "bytes_written": written,
                            "fill_ms": f * 1e3, "fill_gb_s": tensor.numel() * size / f / 1e9, "decode_over_fill": (d / f) if mask else None}
                    print(json.dumps(case))
                    result["cases"].append(case)
                    del tensor, out
    json.dump(result, open(out_path, "w"), indent=1)
    print("wrote " + out_path)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_build_traj.json"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.bench:
        import torch      # (before the context: torch then finds the device the context shares with it)
        assert torch.cuda.is_available(), "--bench needs a GPU: there is no CPU decode to time"
    from oak_amd.engine import Context
    ctx = Context(args.device)
    try:
        if args.bench:
            return bench(ctx, args.out)
        paths = []
        for p in args.paths:
            paths += sorted(glob.glob(os.path.join(p, "*.build.data"))) if os.path.isdir(p) else [p]
        if not paths:
            ap.error("no .build.data files")
        census(ctx, paths)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
