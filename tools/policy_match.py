#!/usr/bin/env python3
"""Does network A play better than network B?  The reference answers with

    vs --budget=0 --bandit=pucb-1.0 --policy-mode=p --p1-eval=A.battle.net --p2-eval=B.battle.net

(cpp/src/vs.cc:107-408: with a zero budget each side samples its policy head's root prior), one game per CPU thread.  This plays the
same matches as batches of whole games resident on the GPU (oak_amd.arena.match) and prints the reference's report.

usage: policy_match.py A.battle.net B.battle.net [--games N] [--teams FILE] [--mirror] [--temp T] [--min M] [--p1-discrete] [--p2-discrete]
                       [--random-p2] [--seed S] [--json out.json]

--games N: matches, as vs counts them (--max-games): two teams are drawn per match and played in both seatings, so 2 N games -- N with
--mirror, where both sides get the same team.  --teams FILE: JSON {"teams": [[[species, move, move, move, move] x 6] ...]} by name, the
layout of tests/golden/ou_sample_teams.json (the default: the reference's 16 sample teams).  --random-p2: B's seat plays uniformly random
legal moves instead (the B path is then ignored).  Output: `score: ... over ... games; Elo diff: ...`, `W D L:` and the three counts, from
A's point of view."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def team_bytes(path):
    from oak_amd import gamedata as G
    teams = json.load(open(path))["teams"]
    return np.array([[[G.match_species(s[0])] + [G.match_move(m) for m in s[1:]] for s in t] for t in teams], dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--teams", default=os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json"))
    ap.add_argument("--mirror", action="store_true")
    ap.add_argument("--temp", type=float, default=1.0)
    ap.add_argument("--min", type=float, default=0.0)
    ap.add_argument("--p1-discrete", action="store_true")
    ap.add_argument("--p2-discrete", action="store_true")
    ap.add_argument("--random-p2", action="store_true")
    ap.add_argument("--seed", type=int, default=0x0A4B)
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    torch.cuda.init()   # torch initialises the GPU before the library does
    from oak_amd import arena
    from oak_amd.engine import Context
    ctx = Context(0)
    res = arena.match(ctx, a.a, None if a.random_p2 else a.b, team_bytes(a.teams), a.games, a.seed, mirror=a.mirror, temp=a.temp, min=a.min,
                      discrete=(a.p1_discrete, a.p2_discrete))
    print("score: %g over %d games; Elo diff: %g" % (res["score"], res["games"], res["elo"]))
    print("W D L:")
    print("%d %d %d" % (res["W"], res["D"], res["L"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(res, a=a.a, b="random" if a.random_p2 else a.b, matches=a.games, mirror=a.mirror, temp=a.temp, min=a.min, seed=a.seed), f)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
