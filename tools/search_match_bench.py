"""Measure matches between two search agents on the forest search (oak_amd.arena.search_games: a batch of games resident on the device, one
forest search per seat and turn, oak_amd/csrc/forestmatch.hip) against the way to play such matches that existed before it: the per-turn host
loop of tools/tutorial_stats.py vs -- tree_search_many per seat on 16 contexts, default batch -- at the same budget, with the same early
stop, over the first --baseline-games of the same games.  The baseline uses only calls that are older than the match loop.

Games: the 16 sample teams (tests/golden/ou_sample_teams.json), two drawn per game, seeds from --seed.  Pairings: pucb_vs_fp (PUCB +
net_default, c 1.5, mode p0.5-e0.5, against UCB + PokeEngine, c 2, mode e) and fp_vs_fp (PokeEngine against PokeEngine), budget --budget,
early stop 10.  Every timed run is a fresh process (this script with --child): it makes its contexts, forest and network, plays a warm-up
(the same batch cut at 2 turns: every allocation and kernel load), then times ONE call with a host clock, the stream idle before and after.
Per pairing and size: --rounds match runs alternated with baseline runs (the baseline's runs are shared by the sizes of a pairing);
reported: the runs, the median, games/s and turn-steps/s (a turn-step = one update of one game), and the schedule counters.  --batch1-games
(0 = skip): one more baseline run at batch = 1, the reference's one-at-a-time order, over that many games, and its ratio to the default batch.
--direction N: PokeEngine against Monte-Carlo, ucb-1.0, mode x, N team pairs in both seatings at --direction-budget, W-D-L next to the
TUTORIAL's 186-1-31 at budget 4,096.  --records: the match runs record both seats' `.battle.data` (search_games(records=True): the two
streams are copied to the host inside the clock); the cells are then named <pairing>/<games>/records.

  python tools/search_match_bench.py [--sizes 256,4096,65536] [--pairings pucb_vs_fp,fp_vs_fp] [--budget 256] [--rounds 3] [--out FILE]
A run that is cut short keeps what it measured: --out is rewritten after every run, and a later run with the same --out goes on from it."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FP = dict(bandit="ucb", c=2.0, evaluator="poke-engine", policy_mode="e")
PAIRINGS = {"pucb_vs_fp": (dict(bandit="pucb", c=1.5, evaluator="net_default.battle.net", policy_mode="p0.5-e0.5"), FP), "fp_vs_fp": (FP, FP)}
EARLY_STOP = 10.0


def draw(n, seed):
    from policy_match import team_bytes
    pool = team_bytes(os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json"))
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(pool), (n, 2))
    teams = np.concatenate([pool[pick[:, 0]].reshape(n, 30), pool[pick[:, 1]].reshape(n, 30)], axis=1).astype(np.uint8)
    return np.ascontiguousarray(teams), rng.integers(0, 1 << 63, n, dtype=np.uint64), rng.integers(0, 1 << 63, n, dtype=np.uint64)


def host_pick(o, side, mode, rng):
    """The baseline's pick from one tree_search output: argmax for mode x, else a sample from the mode's mixture of prior and empirical."""
    emp = np.asarray(o["p2_empirical" if side else "p1_empirical"], dtype=np.float64)
    if mode == "x":
        return int(np.argmax(emp))
    pol = emp + (np.asarray(o["p2_prior" if side else "p1_prior"], dtype=np.float64) if mode.startswith("p") else 0.0)
    return int(rng.choice(len(pol), p=pol / pol.sum()))


def host_loop(ctxs, seats, teams, battle_seeds, seeds, batch, max_turns=1000):
    """tools/tutorial_stats.py vs for these seats, 16 games at a time: per turn and seat one tree_search_many over the games that seat must
    search, the early stop, the update.  Returns (games, turn-steps)."""
    from oak_amd import search as S
    cx, conc, steps = ctxs[0], len(ctxs), 0
    for s0 in range(0, len(seeds), conc):
        n = min(conc, len(seeds) - s0)
        rng = np.random.default_rng(int(seeds[s0]))
        b, dur, r = cx.battle(teams[s0:s0 + n].reshape(n, 2, 6, 5), battle_seeds[s0:s0 + n])
        live = (r & 15) == 0
        ups = np.zeros(n, dtype=int)
        while live.any():
            idx = np.where(live)[0]
            ch = [cx.choices(b[idx], r[idx], 0), cx.choices(b[idx], r[idx], 1)]
            pick, sign = np.zeros((2, len(idx)), dtype=int), np.zeros((2, len(idx)), dtype=int)
            for side in (0, 1):
                need = np.where(ch[side][1] > 1)[0]
                if len(need) == 0:
                    continue
                seat = seats[side]
                outs = S.tree_search_many(ctxs[:len(need)], b[idx[need]], dur[idx[need]], r[idx[need]], rng.integers(1, 2 ** 31, size=len(need)),
                                          iterations=seat["iterations"], c=seat["c"], bandit=seat["bandit"], evaluator=seat["evaluator"],
                                          **({} if batch is None else {"batch": batch}))
                for k, o in zip(need, outs):
                    pick[side][k] = host_pick(o, side, seat["policy_mode"], rng)
                    ev = o["empirical_value"]
                    t = (math.log(ev) if ev > 0 else -math.inf) - (math.log(1 - ev) if ev < 1 else -math.inf)
                    sign[side][k] = 1 if t / EARLY_STOP >= 1 else -1 if t / EARLY_STOP <= -1 else 0
            stop = sign[0] * sign[1] > 0
            live[idx[stop]] = False
            go = np.where(~stop)[0]
            if len(go) == 0:
                continue
            rows = idx[go]
            bb, dd = np.ascontiguousarray(b[rows]), np.ascontiguousarray(dur[rows])
            rr, _ = cx.update(bb, ch[0][0][go, pick[0][go]], ch[1][0][go, pick[1][go]], dd, want_actions=False)
            b[rows], dur[rows], r[rows] = bb, dd, rr
            ups[rows] += 1
            live[rows[((rr & 15) != 0) | (ups[rows] >= max_turns)]] = False
        steps += int(ups.sum())
    return len(seeds), steps


def child(a):
    from oak_amd.arena import search_games
    from oak_amd.engine import Context, Network
    from oak_amd.search import Forest
    if a.child == "direction":
        import torch
        torch.cuda.init()   # search_match builds its battles with torch: torch initialises the GPU before the library does
    ctx = Context(0)
    nets = {}

    def seat(s, budget):
        s = dict(s, iterations=budget)
        if s["evaluator"] not in ("mc", "poke-engine"):
            if s["evaluator"] not in nets:
                nets[s["evaluator"]] = Network(ctx, path=os.path.join(ROOT, "tests", "golden", s["evaluator"]))
            s["evaluator"] = nets[s["evaluator"]]
        return s

    if a.child == "direction":
        from oak_amd.arena import search_match
        from policy_match import team_bytes
        pe, mc = dict(iterations=a.budget, bandit="ucb", c=1.0, evaluator="poke-engine", policy_mode="x"), dict(iterations=a.budget, bandit="ucb", c=1.0, evaluator="mc", policy_mode="x")
        t = time.perf_counter()
        got = search_match(ctx, pe, mc, team_bytes(os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json")), a.games, a.seed, early_stop=0.0, max_turns=300)
        res = dict(form="direction", s=time.perf_counter() - t, budget=a.budget, pairs=a.games, max_turns=300,
                   **{k: got[k] for k in ("W", "D", "L", "games", "score", "stopped")})
        print("RESULT " + json.dumps(res), flush=True)
        return
    seats = tuple(seat(s, a.budget) for s in PAIRINGS[a.pairing])
    teams, battle_seeds, seeds = draw(a.games, a.seed)
    if a.child == "match":
        b, d, r = ctx.battle(teams.reshape(-1, 2, 6, 5), battle_seeds)
        forest = Forest(ctx, a.games, a.budget, contextual=any(s["bandit"] == "pucb" for s in seats))
        kw = dict(forest=forest, early_stop=EARLY_STOP, **({"records": True} if a.records else {}))
        search_games(ctx, seats, b, d, r, seeds, max_turns=2, **kw)
        ctx.synchronize()
        stats = {}
        t = time.perf_counter()
        out = search_games(ctx, seats, b, d, r, seeds, stats=stats, **kw)
        s = time.perf_counter() - t
        res = dict(form="match", s=s, games=a.games, turn_steps=int(out["turns"].sum()), counts=list(out["counts"]),
                   early_stops=int((out["status"] == 3).sum()), **stats)
        if a.records:
            res.update(records=True, record_bytes=[len(x["stream"]) for x in out["records"]])
        forest.close()
    else:
        ctxs = [ctx] + [Context(0) for _ in range(15)]
        warm = tuple(dict(s, iterations=16) for s in seats)
        host_loop(ctxs, warm, teams[:16], battle_seeds[:16], seeds[:16], a.batch or None, max_turns=2)
        t = time.perf_counter()
        games, steps = host_loop(ctxs, seats, teams, battle_seeds, seeds, a.batch or None)
        s = time.perf_counter() - t
        res = dict(form="baseline", s=s, games=games, turn_steps=steps, batch=a.batch or "default")
    res.update(games_per_s=res["games"] / s, turn_steps_per_s=res["turn_steps"] / s)
    print("RESULT " + json.dumps(res), flush=True)


def run_child(form, pairing, games, budget, seed, batch=0, timeout=1100, records=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", form, "--pairing", pairing, "--games", str(games), "--budget", str(budget), "--seed", str(seed),
           "--batch", str(batch)] + (["--records"] if records and form == "match" else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    lines = [x for x in out.stdout.splitlines() if x.startswith("RESULT ")]
    if out.returncode != 0 or not lines:
        raise RuntimeError("child failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="256,4096,65536")
    ap.add_argument("--pairings", default="pucb_vs_fp,fp_vs_fp")
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-games", type=int, default=256)
    ap.add_argument("--batch1-games", type=int, default=16)
    ap.add_argument("--direction", type=int, default=0)
    ap.add_argument("--direction-budget", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0x0A4B)
    ap.add_argument("--max-seconds", type=float, default=1e9)
    ap.add_argument("--out")
    ap.add_argument("--records", action="store_true")
    ap.add_argument("--child", choices=("match", "baseline", "direction"))
    ap.add_argument("--pairing", default="fp_vs_fp")
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--batch", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    t_begin = time.perf_counter()
    res = {"what": "tools/search_match_bench.py on one MI355X", "budget": a.budget, "rounds": a.rounds, "early_stop": EARLY_STOP,
           "timing": "every run a fresh process; a host clock around one call after a warm-up, the stream idle before and after",
           "match": "search_games, host arrays in and out, a Forest made before the clock starts",
           "baseline": "the per-turn host loop of tools/tutorial_stats.py vs: tree_search_many per seat on 16 contexts, default batch, the first %d of the "
                       "same games, the same budget and early stop" % a.baseline_games,
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
    for pairing in a.pairings.split(","):
        base = res["cells"].setdefault(pairing + "/baseline", {"runs": []})
        for n in sizes:
            cell = res["cells"].setdefault("%s/%d%s" % (pairing, n, "/records" if a.records else ""), {"pairing": pairing, "games": n, "runs": []})
            for k in range(a.rounds):
                for which in (("match", "baseline") if k % 2 == 0 else ("baseline", "match")):
                    if late():
                        continue
                    if which == "match" and len(cell["runs"]) <= k:
                        cell["runs"].append(run_child("match", pairing, n, a.budget, a.seed, records=a.records))
                        print("  %s N=%d match run %d: %.2f s, %.1f games/s" % (pairing, n, k, cell["runs"][-1]["s"], cell["runs"][-1]["games_per_s"]), file=sys.stderr, flush=True)
                    if which == "baseline" and len(base["runs"]) <= k:
                        base["runs"].append(run_child("baseline", pairing, a.baseline_games, a.budget, a.seed))
                        print("  %s baseline run %d: %.2f s, %.1f games/s" % (pairing, k, base["runs"][-1]["s"], base["runs"][-1]["games_per_s"]), file=sys.stderr, flush=True)
                    save()
            if cell["runs"]:
                med = float(np.median([x["s"] for x in cell["runs"]]))
                cell.update(median_s=med, games_per_s=cell["runs"][0]["games"] / med, turn_steps_per_s=cell["runs"][0]["turn_steps"] / med)
                if base["runs"]:
                    best = max(x["games_per_s"] for x in base["runs"])
                    base.update(median_games_per_s=float(np.median([x["games_per_s"] for x in base["runs"]])), fastest_games_per_s=best)
                    cell["match_median_beats_baseline_fastest"] = bool(cell["games_per_s"] > best)
            save()
        if a.batch1_games and base["runs"] and "batch1" not in base and not late():
            base["batch1"] = run_child("baseline", pairing, a.batch1_games, a.budget, a.seed, batch=1)
            base["default_batch_over_batch1_games_per_s"] = base["median_games_per_s"] / base["batch1"]["games_per_s"]
            save()
    if a.direction and "direction" not in res and not late():
        got = run_child("direction", "fp_vs_fp", a.direction, a.direction_budget, a.seed)
        res["direction"] = dict(got, what="PokeEngine (agent A) against Monte-Carlo, ucb-1.0, mode x, both seatings, no early stop; W D L from A's side",
                                tutorial={"W": 186, "D": 1, "L": 31, "budget": 4096, "where": "TUTORIAL.md:99-104"})
        save()
    claim = [res["cells"].get("%s/4096" % p, {}).get("match_median_beats_baseline_fastest") for p in a.pairings.split(",")]
    res["claim"] = "at 4,096 games the match loop's median games/s beats the baseline's fastest run: " + ", ".join(
        "%s: %s" % (p, "not measured" if c is None else c) for p, c in zip(a.pairings.split(","), claim))
    save()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
