"""What a round of the loop pays between self-play and the first training batch, with the replay window and without it (not gated).

  python tools/replay_window_bench.py [--games 4096] [--budget 64] [--window 65536] [--rows 65536] [--out profiles/r34_replay_window.json]

One self-play batch (UCB + PokeEngine) is generated once and kept on the device.  A window of --window records is filled with copies of it.
Then, alternating in one process, medians of three:
  window  : ReplayWindow.append(stream, offsets) of the batch to the full window, and the first sample of --rows rows;
  rebuild : what the library offered before the window for the same result -- the batch's records to the host, concatenated with the kept
            window's newest records, FrameCorpus(ctx, bytes) (host index, upload of everything), and the first sample.
Both end with a wait for the device.  Reported with the bytes each path moves between host and device and the host reads it makes, and the
per-round split generate / append / train of oak_amd.rl.run at --games games (PokeEngine self-play, 16 steps of 4,096 rows)."""
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
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--budget", type=int, default=64)
    ap.add_argument("--window", type=int, default=65536)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r34_replay_window.json"))
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda:0")
    from oak_amd import rl
    from oak_amd.engine import Context
    from oak_amd.search import Forest
    from oak_amd.train import EncodedBattleFrames, FrameCorpus, ReplayWindow
    from policy_match import team_bytes
    ctx = Context(0)
    pool = team_bytes(os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json")).reshape(-1, 30)
    forest = Forest(ctx, a.games, a.budget)
    t0 = time.perf_counter()
    out = rl.selfplay_round(ctx, forest, "poke-engine", pool, a.games, 34, 0, a.budget, bandit="ucb-2.0")
    torch.cuda.synchronize()
    generate_s = time.perf_counter() - t0
    forest.close()
    stream, offsets = out[0], out[1]
    kept_games = int((out[4] == 0).sum().item())
    batch_bytes = int(stream.numel())
    enc = EncodedBattleFrames(a.rows, "cuda:0")
    window = ReplayWindow(ctx, a.window, 1 << 40)
    while window.append(stream, offsets)["evicted"] == 0:
        pass
    kept = window.records()                       # the full window on the host, for the rebuild path
    # the newest (window - batch) records' bytes: found once, outside the timing (a loop that keeps its window on the host knows them)
    from oak_amd.frames import replay_index
    idx = replay_index(kept)
    tail_from = int(idx["offsets"][kept_games]) if kept_games < len(idx["offsets"]) else len(kept)

    def run_window():
        t = time.perf_counter()
        window.append(stream, offsets)
        t1 = time.perf_counter()
        window.sample(enc, 1, 0, 1, count_ok=False)
        torch.cuda.synchronize()
        return t1 - t, time.perf_counter() - t1

    def run_rebuild():
        t = time.perf_counter()
        host = stream.cpu().numpy().tobytes()
        data = kept[tail_from:] + host
        t1 = time.perf_counter()
        corpus = FrameCorpus(ctx, data)
        t2 = time.perf_counter()
        corpus.sample(enc, 1, 0, 1, count_ok=False)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        n = corpus.info()["records"]
        corpus.close()
        return t1 - t, t2 - t1, t3 - t2, len(data), n

    run_window(), run_rebuild()                  # warm: allocations, the first launch of every kernel
    w, r = [], []
    for _ in range(3):
        w.append(run_window())
        r.append(run_rebuild())
    med = lambda xs: float(np.median(xs))
    n_slices = int(offsets.numel()) - 1
    res = {
        "games": a.games, "budget": a.budget, "kept_games": kept_games, "batch_bytes": batch_bytes, "generate_s": generate_s,
        "window_records": window.stats()["records"], "window_bytes": window.stats()["bytes"], "rows": a.rows,
        "window": {"append_ms": [1e3 * x[0] for x in w], "first_sample_ms": [1e3 * x[1] for x in w], "total_ms_median": 1e3 * med([x[0] + x[1] for x in w]),
                   "host_reads": 2, "bytes_device_to_host": 40 + 3 * n_slices + 4, "bytes_host_to_device": 0,
                   "note": "reads: the append's summary with the batch's frames and classes, and the eligible count E"},
        "rebuild": {"to_host_and_concat_ms": [1e3 * x[0] for x in r], "corpus_create_ms": [1e3 * x[1] for x in r], "first_sample_ms": [1e3 * x[2] for x in r],
                    "total_ms_median": 1e3 * med([x[0] + x[1] + x[2] for x in r]), "host_reads": 2,
                    "bytes_device_to_host": batch_bytes + 4 * r[0][4], "bytes_host_to_device": r[0][3] + (8 + 2 + 1 + 4) * r[0][4],
                    "note": "reads: the batch's records and the valid-frame counts; up: every record, the index arrays and the eligible list"},
    }
    res["speedup"] = res["rebuild"]["total_ms_median"] / res["window"]["total_ms_median"]
    window.close()
    if not a.no_loop:
        rows = []
        net = open(os.path.join(ROOT, "tests", "golden", "net_default.battle.net"), "rb").read()
        rl.run(ctx, net, pool, 3, a.games, a.budget, 16, 4096, 1e-3, a.window, max_bytes=1 << 40, bandit="ucb-2.0", evaluator="poke-engine", seed=34, log=rows.append)
        res["rl_loop_rounds"] = [{k: row[k] for k in ("round", "games", "frames", "window", "generate_s", "append_s", "train_s")} for row in rows]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
