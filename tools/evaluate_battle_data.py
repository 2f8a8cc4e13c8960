"""Score a network on held-out `.battle.data` games: its value and policy on every frame of every record, evaluated on the GPU
(oak_amd.train.FrameCorpus.evaluate; the rules are in include/oakgpu.h), and the loss terms battle.py would report for them.

  python tools/evaluate_battle_data.py PATH... --network X [--discrete] [--value-nash-weight W] [--value-empirical-weight W]
         [--value-score-weight W] [--p-nash-weight W] [--policy-loss-weight W] [--min-iterations N] [--chunk-mb N] [--chunk-rows N]
         [--per-record] [--json OUT]

PATH: files, or directories whose `*.battle.data` files (recursively, sorted) are read the way tools/verify_battle_data.py reads them:
small files packed into one upload up to --chunk-mb, large ones read in pieces that end on record boundaries.  Prints one JSON summary:
mse, ce_p1, ce_p2 (means over the rows evaluated) and loss = mse + policy_loss_weight * (ce_p1 + ce_p2); rows evaluated, excluded (their
iterations are below --min-iterations) and failed (rows that are not OK: see the replay check); wall time and frames / s.  The sums are
added record by record in file order, so the figures do not depend on --chunk-mb or --chunk-rows.  --per-record adds every record's
sums and counts.  Exit status 0, or 2 on unreadable input."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from verify_battle_data import _paths  # noqa: E402  (the same PATH rule)


def evaluate_files(ctx, net, paths, weights, min_iterations=1, chunk_bytes=256 << 20, chunk_rows=0, per_record=False):
    """FrameCorpus.evaluate over many files: {"sq_err", "ce1", "ce2", "rows", "excluded", "failed", "records", "stopped", "per_record"}."""
    from oak_amd.frames import _whole_records
    from oak_amd.train import FrameCorpus
    tot = {"sq_err": 0.0, "ce1": 0.0, "ce2": 0.0, "rows": 0, "excluded": 0, "failed": 0, "records": 0, "malformed": 0, "stopped": [], "per_record": []}
    pend = []

    def flush():
        if not pend:
            return
        corpus = FrameCorpus(ctx, b"".join(pend))
        try:
            tot["malformed"] += corpus.info()["malformed"]
            res = corpus.evaluate(net, *weights, min_iterations=min_iterations, chunk_rows=chunk_rows, per_record=True)
        finally:
            corpus.close()
        for rec in res["records"]:                                      # record order: independent of the packing
            for name in ("sq_err", "ce1", "ce2", "rows", "excluded", "failed"):
                tot[name] += rec[name]
        tot["records"] += len(res["records"])
        if per_record:
            tot["per_record"] += [{name: rec[name] for name in ("sq_err", "ce1", "ce2", "rows", "excluded", "failed")} for rec in res["records"]]
        pend.clear()

    for path in paths:
        with open(path, "rb") as f:
            for off, piece in _whole_records(f, chunk_bytes):
                if not piece:
                    if off is not None:
                        tot["stopped"].append({"file": str(path), "offset": off})
                    continue
                if pend and sum(len(p) for p in pend) + len(piece) > chunk_bytes:
                    flush()
                pend.append(piece)
    flush()
    return tot


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--network", required=True)
    ap.add_argument("--discrete", action="store_true")
    ap.add_argument("--value-nash-weight", type=float, default=0.0)
    ap.add_argument("--value-empirical-weight", type=float, default=0.5)
    ap.add_argument("--value-score-weight", type=float, default=0.5)
    ap.add_argument("--p-nash-weight", type=float, default=0.5)
    ap.add_argument("--policy-loss-weight", type=float, default=1.0)
    ap.add_argument("--min-iterations", type=int, default=1)
    ap.add_argument("--chunk-mb", type=float, default=256)
    ap.add_argument("--chunk-rows", type=int, default=0)
    ap.add_argument("--per-record", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args(argv)
    from oak_amd import _lib
    try:
        paths = _paths(a.paths)
        for p in paths + [a.network]:
            with open(p, "rb"):
                pass
    except OSError as e:
        print(json.dumps({"error": "unreadable input: %s" % e}))
        return 2
    from oak_amd.engine import Context, Network
    ctx = Context(0)
    net = Network(ctx, path=a.network, discrete=a.discrete)
    weights = (a.value_nash_weight, a.value_empirical_weight, a.value_score_weight, a.p_nash_weight)
    t0 = time.perf_counter()
    tot = evaluate_files(ctx, net, paths, weights, a.min_iterations, int(a.chunk_mb * (1 << 20)), a.chunk_rows, a.per_record)
    wall = time.perf_counter() - t0
    rows = tot["rows"]
    mean = lambda x: x / rows if rows else 0.0
    frames = rows + tot["excluded"] + tot["failed"]
    summary = {"library": _lib.LIB_PATH, "network": a.network, "discrete": a.discrete, "files": len(paths), "records": tot["records"],
               "malformed": tot["malformed"], "stopped": tot["stopped"],
               "weights": {"value_nash": weights[0], "value_empirical": weights[1], "value_score": weights[2], "p_nash": weights[3],
                           "policy_loss": a.policy_loss_weight, "min_iterations": a.min_iterations},
               "mse": mean(tot["sq_err"]), "ce_p1": mean(tot["ce1"]), "ce_p2": mean(tot["ce2"]),
               "loss": mean(tot["sq_err"]) + a.policy_loss_weight * (mean(tot["ce1"]) + mean(tot["ce2"])),
               "sums": {"sq_err": tot["sq_err"], "ce1": tot["ce1"], "ce2": tot["ce2"]},
               "rows": rows, "excluded": tot["excluded"], "failed": tot["failed"], "frames": frames,
               "wall_s": wall, "frames_per_s": frames / wall if wall > 0 else None}
    if a.per_record:
        summary["per_record"] = tot["per_record"]
    text = json.dumps(summary, indent=1)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")
    print(text if not a.per_record else json.dumps({k: v for k, v in summary.items() if k != "per_record"}, indent=1))
    net = None
    return 0


if __name__ == "__main__":
    sys.exit(main())
