"""Measure what skipped battles (generate's --battle-skip-prob / --t1-budget; oak_amd.frames.forest_selfplay's built / battle_skip_prob /
t1_budget) cost and buy the device game loop as a source of build data, and what BuildWindow.append costs against rebuilding a corpus.

One process, one MI355X, UCB + PokeEngine, every game built on both seats (build.provide_pairs with a random `.build.net`, every team
modified), --budget iterations = t1_budget, battle_skip_prob in --probs; probability 0 IS the loop as it was before the fields existed.
A forest made once, a warm-up (every probability under a length cap of 2 frames), then --rounds rounds that alternate the probabilities,
each run ONE forest_selfplay call on device tensors timed with a host clock, the stream idle before and after, followed by
build.game_records and BuildWindow.append (timed on their own) into a window of --window records.  Recorded per run: seconds per call, build
records per second of the call, battle frames per second, rows searched, the append's seconds; per probability the medians; and once per
probability the seconds of the rebuild the library offered before the window: the batch's records to the host, joined to the held bytes,
cut to the window, TrajectoryCorpus(ctx, bytes).

  python tools/build_loop_bench.py [--games 4096] [--budget 256] [--probs 0,0.5,0.9] [--rounds 3] [--window 65536] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--probs", default="0,0.5,0.9")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=0x0A4B)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda:0")                                      # (torch initialises the GPU before the library does)
    from oak_amd import build, netfile
    from oak_amd.engine import Context
    from oak_amd.frames import forest_selfplay
    from oak_amd.search import Forest
    from policy_match import team_bytes
    probs = [float(p) for p in a.probs.split(",")]
    dev = torch.device("cuda:0")
    ctx = Context(0)
    pool = team_bytes(os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json")).reshape(-1, 30)
    rng = np.random.default_rng(a.seed)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.build.net")
        netfile.write_random_build_net(path, 7)
        with build.BuildNetwork(ctx, path) as net:
            teams, seats = build.provide_pairs(ctx, net, pool, rng.integers(0, 1 << 63, (a.games, 2), dtype=np.uint64), team_modify_prob=1.0,
                                               pokemon_delete_prob=0.2, move_delete_prob=0.2)
    built = ((seats[0]["n_updates"] > 0) | ((seats[1]["n_updates"] > 0) << 1)).astype(np.uint8)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int16) if x.dtype == np.uint16 else np.ascontiguousarray(x)).to(dev)
    dseats = tuple({k: up(s[k]) for k in ("teams_init", "sizes", "n_updates", "action", "prob")} for s in seats)
    d_teams, d_built = up(teams), up(built)
    d_bs, d_sd = (up(rng.integers(0, 1 << 63, a.games, dtype=np.uint64).view(np.int64)) for _ in range(2))
    forest = Forest(ctx, a.games, a.budget)
    kw = dict(c=2.0, bandit="ucb", evaluator="poke-engine", policy_mode="e", forest=forest, solve_nash="device", built=d_built, t1_budget=a.budget)
    window = build.BuildWindow(ctx, a.window)
    res = {"what": "tools/build_loop_bench.py on one MI355X", "games": a.games, "budget": a.budget, "t1_budget": a.budget, "rounds": a.rounds, "window": a.window,
           "games_with_both_seats_built": int((built == 3).sum()), "games_with_a_built_seat": int((built != 0).sum()),
           "timing": "one process; a host clock around one forest_selfplay call on device tensors after a warm-up, the stream idle before and after; the "
                     "probabilities alternate; game_records + BuildWindow.append timed on their own, synchronised",
           "baseline": "battle_skip_prob 0 is the loop as it was before the fields existed", "probs": {}}

    def run(prob):
        torch.cuda.synchronize()
        ctx.synchronize()
        stats = {}
        t = time.perf_counter()
        out = forest_selfplay(ctx, d_teams, d_bs, d_sd, a.budget, stats=stats, battle_skip_prob=prob, **kw)
        torch.cuda.synchronize()
        s = time.perf_counter() - t
        t = time.perf_counter()
        records, count = build.game_records(ctx, dseats, out[4], out[3], stats["matchup"])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        window.append(records, count)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        n = int(count.item())
        r = dict(s=s, played=int((out[4] == 0).sum().item()), skipped=int((out[4] == 3).sum().item()), frames=int(out[2].sum().item()), rows=stats["rows"],
                 turns=stats["turns"], launched=stats["launched"], run=stats["run"], build_records=n, game_records_s=t1 - t, append_s=t2 - t1)
        r.update(build_records_per_s=n / s, frames_per_s=r["frames"] / s)
        print("  prob %g: %.2f s, %d played, %d skipped, %d frames, %d rows, %d build records, append %.2f ms" % (
            prob, s, r["played"], r["skipped"], r["frames"], r["rows"], n, 1e3 * r["append_s"]), file=sys.stderr, flush=True)
        return r, records, n

    for prob in probs:
        forest_selfplay(ctx, d_teams, d_bs, d_sd, a.budget, max_battle_length=2, battle_skip_prob=prob, **kw)
    cells = {prob: {"runs": []} for prob in probs}
    for k in range(a.rounds):
        for prob in (probs if k % 2 == 0 else probs[::-1]):
            r, records, n = run(prob)
            cells[prob]["runs"].append(r)
            if "rebuild_s" not in cells[prob]:       # what the window replaces: records down, joined, cut, a corpus made again
                held = window.records()
                torch.cuda.synchronize()
                t = time.perf_counter()
                new = records.reshape(-1)[:n * build.RECORD_BYTES].cpu().numpy().tobytes()
                data = (held + new)[-a.window * build.RECORD_BYTES:]
                corpus = build.TrajectoryCorpus(ctx, data)
                ctx.synchronize()
                cells[prob]["rebuild_s"] = time.perf_counter() - t
                cells[prob]["rebuild_records"] = len(data) // build.RECORD_BYTES
                corpus.close()
    for prob, c in cells.items():
        runs = c["runs"]
        mid = sorted(runs, key=lambda x: x["s"])[len(runs) // 2]
        c.update(median_s=float(np.median([x["s"] for x in runs])), median_append_s=float(np.median([x["append_s"] for x in runs])),
                 median_game_records_s=float(np.median([x["game_records_s"] for x in runs])), rows=mid["rows"], frames=mid["frames"], skipped=mid["skipped"],
                 build_records=mid["build_records"], build_records_per_s=mid["build_records_per_s"], frames_per_s=mid["frames_per_s"])
        res["probs"]["%g" % prob] = c
    base = res["probs"].get("0")
    if base:
        for c in res["probs"].values():
            c.update(time_ratio_over_prob_0=c["median_s"] / base["median_s"], rows_ratio_over_prob_0=c["rows"] / base["rows"],
                     build_records_per_s_ratio_over_prob_0=c["build_records_per_s"] / base["build_records_per_s"])
    res["window_stats"] = window.stats()
    window.close()
    forest.close()
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
