"""Measure the evaluation of a network on every frame of a `.battle.data` corpus (FrameCorpus.evaluate / inference) against the route
that existed before it: a loop of pyoak.cpp_inference per record, one zero-iteration search per frame.

Corpus: tools/replay_bench.py's seeded random-play games (built on the GPU), every frame given random iterations, values and
probabilities, tiled on the host until it holds --min-frames frames.  Reported: FrameCorpus.evaluate on the resident corpus (device
events on the context's stream around the call, after a warm-up call, --repeats times, for several chunk sizes), FrameCorpus.inference
into host arrays, tools/evaluate_battle_data.py's path end to end from 8 files, and the old route on as many records as fit in
--old-seconds; one record's values and logits are compared between the two routes.

  python tools/corpus_inference_bench.py [--games 8192] [--min-frames 2e6] [--repeats 5] [--old-seconds 45] [--out profiles/r10_corpus_inference.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def with_targets(buf, offs, frames, lengths, seed=5):
    """Every byte of every frame behind its (m | n, c1, c2) head drawn at random: iterations, values, probabilities."""
    n, T = len(lengths), frames.shape[0]
    valid = np.arange(T)[:, None] < lengths[None, :]
    fsz = np.where(valid, 11 + 4 * (frames[..., 0].astype(np.int64) + frames[..., 1]), 0)
    fpos = offs[None, :] + 391 + np.concatenate([np.zeros((1, n), np.int64), np.cumsum(fsz, 0)[:-1]], 0)
    fp = fpos[valid]
    keep = np.zeros(buf.size, dtype=bool)
    keep[(offs[:, None] + np.arange(391)[None, :]).ravel()] = True
    for k in range(3):
        keep[fp + k] = True
    rand = np.random.default_rng(seed).integers(0, 256, buf.size, dtype=np.uint8)
    return np.where(keep, buf, rand)


def main():
    import torch
    from oak_amd.engine import Context, Network
    from oak_amd.train import FrameCorpus
    from replay_bench import assemble, play_corpus
    from evaluate_battle_data import evaluate_files
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=8192)
    ap.add_argument("--min-frames", type=float, default=2e6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--old-seconds", type=float, default=45)
    ap.add_argument("--network", default=os.path.join(ROOT, "tests", "golden", "net_default.battle.net"))
    ap.add_argument("--out")
    a = ap.parse_args()
    torch.cuda.init()   # torch initialises the GPU before the library does
    ctx = Context(0)
    first, results, frames, lengths = play_corpus(ctx, a.games, ghost_frac=0.0)
    buf, offs = assemble(first, results, frames, lengths)
    buf = with_targets(buf, offs, frames, lengths)
    n, total = len(offs), int(lengths.sum())
    tiles = max(1, int(np.ceil(a.min_frames / total)))
    data = buf.tobytes() * tiles
    rows = total * tiles
    res = {"what": "tools/corpus_inference_bench.py on one MI355X", "network": os.path.basename(a.network), "games": n, "frames": total, "tiles": tiles,
           "records": n * tiles, "rows": rows, "bytes": len(data), "max_frames": int(lengths.max()),
           "note": "the corpus is the same %d random-play games repeated %d times; targets are random bytes" % (n, tiles)}
    net = Network(ctx, path=a.network)
    corpus = FrameCorpus(ctx, data)
    w = (0.25, 0.25, 0.5, 0.25)
    warm = corpus.evaluate(net, *w, min_iterations=1)
    assert warm["failed"] == 0 and warm["rows"] + warm["excluded"] == rows, warm
    res["losses"] = {k: warm[k] for k in ("mse", "ce_p1", "ce_p2", "rows", "excluded", "failed")}
    stream = torch.cuda.ExternalStream(ctx.lib.oakgpu_get_stream(ctx.handle))
    res["evaluate"] = {}
    for chunk_rows in (65536, 16384, 262144, 1048576):
        corpus.evaluate(net, *w, chunk_rows=chunk_rows)                 # (warm-up of this shape: the workspace grows once)
        ms = []
        for _ in range(a.repeats if chunk_rows == 65536 else 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.synchronize()
            t = time.perf_counter()
            e0.record(stream)
            got = corpus.evaluate(net, *w, chunk_rows=chunk_rows)
            e1.record(stream)
            e1.synchronize()
            ms.append((e0.elapsed_time(e1), (time.perf_counter() - t) * 1e3))
            assert (got["sq_err"], got["ce1"], got["ce2"]) == (warm["sq_err"], warm["ce1"], warm["ce2"])   # the chunking changes no bit
        dev = [x[0] for x in ms]
        res["evaluate"][str(chunk_rows)] = {"device_ms": dev, "host_wall_ms": [x[1] for x in ms], "median_ms": float(np.median(dev)),
                                            "frames_per_s_median": rows / (float(np.median(dev)) / 1e3),
                                            "spread_pct": 100 * (max(dev) - min(dev)) / float(np.median(dev))}
    res["evaluate"]["timing"] = ("device events on the context's stream around FrameCorpus.evaluate (the host form: per chunk the walk, the "
                                 "leaf evaluator, the terms, the record sums, a copy of the sums and a wait), after a warm-up call of the same shape")
    corpus.inference(net, records=(0, n))
    t = time.perf_counter()
    out = corpus.inference(net)
    ti = time.perf_counter() - t
    res["inference_host_arrays"] = {"s": ti, "frames_per_s": rows / ti, "what": "FrameCorpus.inference into numpy arrays: the copies back included (166 B per row)"}
    # end to end from files
    with tempfile.TemporaryDirectory() as td:
        cut = np.linspace(0, n, 9).astype(int)
        paths = []
        for i in range(8):
            lo = int(offs[cut[i]])
            hi = int(offs[cut[i + 1]]) if cut[i + 1] < n else buf.size
            p = os.path.join(td, "part%d.battle.data" % i)
            buf[lo:hi].tofile(p)
            paths.append(p)
        evaluate_files(ctx, net, paths[:1], w)
        t = time.perf_counter()
        tot = evaluate_files(ctx, net, paths, w)
        te = time.perf_counter() - t
        assert tot["rows"] + tot["excluded"] == total and tot["failed"] == 0
    res["end_to_end_files"] = {"files": 8, "frames": total, "s": te, "frames_per_s": total / te,
                               "what": "tools/evaluate_battle_data.py's path on the untiled corpus: read, index, upload, evaluate, per-record sums added in Python"}
    # the old route: pyoak.cpp_inference per record (its own context in this process)
    from oak_amd import pyoak
    recs = [data[int(offs[r]):int(offs[r + 1]) if r + 1 < n else buf.size] for r in range(n)]
    pyoak.cpp_inference(recs[0], a.network)
    t, done, old_frames, first_old = time.perf_counter(), 0, 0, None
    while done < n and time.perf_counter() - t < a.old_seconds:
        o = pyoak.cpp_inference(recs[done], a.network)
        first_old = o if first_old is None else first_old
        old_frames += int(lengths[done])
        done += 1
    to = time.perf_counter() - t
    res["old_route"] = {"records": done, "frames": old_frames, "s": to, "frames_per_s": old_frames / to,
                        "what": "a loop of pyoak.cpp_inference per record: one zero-iteration search and one update call per frame"}
    lo, hi = 0, int(lengths[0])
    same = (first_old["value"].tobytes() == out.value[lo:hi, 0].tobytes() and first_old["policy_logit"].tobytes() == out.policy_logit[lo:hi].tobytes())
    res["old_route"]["record_0_value_and_logits_identical"] = bool(same)
    res["ratio_evaluate_over_old"] = res["evaluate"]["65536"]["frames_per_s_median"] / res["old_route"]["frames_per_s"]
    res["ratio_end_to_end_over_old"] = res["end_to_end_files"]["frames_per_s"] / res["old_route"]["frames_per_s"]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
