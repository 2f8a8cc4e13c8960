"""Measure the training-batch loader (oak_amd.train: oakgpu_frames_sample_dev and what it is made of) on an MI355X.

Corpora: (a) tools/replay_bench.py's seeded random-play corpus, played on the device and tiled (the same games repeated) up to
--min-frames frames; (b) --selfplay-games self-play records (real iterations and probabilities; short searches).  Per corpus and batch
size (4,096 and 65,536 rows), HIP-event time on the context's stream, after warm-up, the cases alternated over --repeats rounds,
median and spread reported:
  sample   oakgpu_frames_sample_dev: k_frames_draw + k_frames_order + k_frames_pick + k_frames_encode
  encode   oakgpu_frames_encode_dev on the same picks: the same without k_frames_draw
  rows     oakgpu_encode_battles_dev on as many states: k_frames_requests + k_frames_encode, i.e. the row writer without the walk
so that walk ~ encode - rows and draw ~ sample - encode (differences of medians, not kernel timers: the per-kernel split a profiler gives
is `rocprofv3 --kernel-trace --stats -- python tools/train_frames_bench.py --repeats 3`).  `rows` -- k_frames_encode together with the
small k_frames_requests in front of it, so an upper bound of k_frames_encode alone -- is held against its HBM floor, the bytes that call
writes (11,530 per row: pokemon, active, hp, choice_indices, k; a sampled row has 167 more in targets, status and where) at the 6.3 TB/s
a streaming kernel reaches on this part; `walk` against the longest picked prefix times the lone-wave turn-step time of DESIGN.md 9 (a
batch is latency bound by its longest prefix).

  python tools/train_frames_bench.py [--games 4096] [--min-frames 2e6] [--selfplay-games 4] [--repeats 7] [--out profiles/r09_train_frames.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oak_amd import _lib  # noqa: E402

POSITION_ROW_BYTES = 4 * (2 * 6 * 198 + 2 * 229 + 12) + 8 * 18 + 2          # what `rows` writes: pokemon, active, hp, choice_indices, k
ROW_BYTES = POSITION_ROW_BYTES + 4 * (18 + 18 + 3) + 2 + 4 + 1 + 4           # a sampled row: + policies, values, score, choice, iterations, status, where
HBM_STREAM_BPS = 6.3e12       # measured float4 copy rate of the part (8.0 TB/s spec)
LONE_WAVE_TURN_US = 6.4       # a dense lone wave's turn-step on the register engine (k_tree_step_staged)


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    med = float(np.median(ms))
    return {"ms": [float(x) for x in ms], "median_ms": med, "spread_pct": 100 * (max(ms) - min(ms)) / med}


def measure(ctx, name, data, sizes, repeats, min_iterations):
    import torch
    from oak_amd.train import EncodedBattleFrames, FrameCorpus
    dev = torch.device("cuda", 0)
    lib, h = ctx.lib, ctx.handle
    stream = torch.cuda.ExternalStream(lib.oakgpu_get_stream(h))
    corpus = FrameCorpus(ctx, data)
    out = {"corpus": name, "info": corpus.info(), "bytes": len(data), "min_iterations": min_iterations, "batches": {}}
    encs = {n: EncodedBattleFrames(n, dev) for n in sizes}
    ptrs = {n: encs[n].pointers() for n in sizes}
    results = {n: torch.zeros(n, dtype=torch.uint8, device=dev) for n in sizes}
    snaps, cases = {}, []
    for n in sizes:
        e = encs[n]
        assert corpus.sample(e, 1, 0, min_iterations) == n          # warm-up: workspace, valid-frame counts, eligible list
        frames = e.picks.view(torch.int32)[:, 1]
        snaps[n] = {"longest_prefix": int(frames.max()), "mean_prefix": float(frames.float().mean())}
        # states for `rows`: the first n stored battles of the corpus stand in for the snapshots (the writer's cost does not depend on them)
        b = np.frombuffer(data, np.uint8, 384, 6)
        e.b = torch.from_numpy(np.tile(b, (n, 1))).to(dev)
        e.d = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
        cases += [("sample", n), ("encode", n), ("rows", n)]
    torch.cuda.synchronize()

    def run(kind, n, seed):
        e = encs[n]
        if kind == "sample":
            _lib.check(lib.oakgpu_frames_sample_dev(h, corpus.handle, n, seed, 0, min_iterations, e.picks.data_ptr(), C.byref(ptrs[n])))
        elif kind == "encode":
            _lib.check(lib.oakgpu_frames_encode_dev(h, corpus.handle, e.picks.data_ptr(), n, C.byref(ptrs[n])))
        else:
            _lib.check(lib.oakgpu_encode_battles_dev(h, e.b.data_ptr(), e.d.data_ptr(), results[n].data_ptr(), n, e.pokemon.data_ptr(), e.active.data_ptr(),
                                                     e.hp.data_ptr(), e.choice_indices.data_ptr(), e.k.data_ptr()))
    ms = {c: [] for c in cases}
    for rep in range(repeats + 1):                                    # round 0 is warm-up; the cases alternate inside a round
        for c in cases:
            t = timed(stream, lambda: run(c[0], c[1], 1))
            if rep:
                ms[c].append(t)
    for n in sizes:
        s, e, r = (stats(ms[(kind, n)]) for kind in ("sample", "encode", "rows"))
        walk_ms = e["median_ms"] - r["median_ms"]
        floor_ms = n * POSITION_ROW_BYTES / HBM_STREAM_BPS * 1e3
        bound_ms = snaps[n]["longest_prefix"] * LONE_WAVE_TURN_US * 1e-3
        out["batches"][str(n)] = {
            "rows": n, **snaps[n], "sample": s, "encode": e, "rows_only": r, "rows_per_s_sample": n / (s["median_ms"] * 1e-3),
            "draw_ms_by_difference": s["median_ms"] - e["median_ms"], "walk_ms_by_difference": walk_ms,
            "rows_only_bytes": n * POSITION_ROW_BYTES, "rows_only_hbm_floor_ms": floor_ms, "rows_only_over_floor": r["median_ms"] / floor_ms,
            "walk_bound_ms_longest_prefix_x_lone_wave_turn": bound_ms, "walk_over_bound": walk_ms / bound_ms if bound_ms else None}
    corpus.close()
    return out


def main():
    import torch
    from oak_amd.engine import Context
    import replay_bench as RB
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--min-frames", type=float, default=2e6)
    ap.add_argument("--selfplay-games", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    torch.cuda.init()   # torch initialises the GPU before the library does
    ctx = Context(0)
    res = {"row_bytes": ROW_BYTES, "position_row_bytes": POSITION_ROW_BYTES, "hbm_stream_bytes_per_s": HBM_STREAM_BPS, "lone_wave_turn_us": LONE_WAVE_TURN_US, "repeats": a.repeats,
           "timing": "HIP events on the context's stream around each call, one warm-up round, cases alternated inside every round", "corpora": []}
    first, results, frames, lengths = RB.play_corpus(ctx, a.games)
    buf, _ = RB.assemble(first, results, frames, lengths)
    tiles = max(1, int(np.ceil(a.min_frames / int(lengths.sum()))))
    res["corpora"].append(measure(ctx, "random play, %d games tiled %d times" % (a.games, tiles), np.tile(buf, tiles).tobytes(), (4096, 65536), a.repeats, 0))
    if a.selfplay_games:
        from oak_amd.frames import selfplay_game
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_oracle_goldens import benchmark_teams
        teams = np.array(benchmark_teams(), dtype=np.uint8)
        recs = [selfplay_game(ctx, teams, battle_seed=7000 + g, iterations=256, batch=256, seed=g + 1)[0] for g in range(a.selfplay_games)]
        res["corpora"].append(measure(ctx, "self-play, %d games of 256 iterations a turn" % a.selfplay_games, b"".join(recs), (4096, 65536), a.repeats, 1))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
