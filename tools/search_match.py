#!/usr/bin/env python3
"""Does agent A play better than agent B when both SEARCH?  The reference answers with

    vs --p1-budget=1024 --p1-bandit=pucb-1.5 --p1-eval=A.battle.net --p2-budget=4096 --p2-bandit=ucb-1.0 --p2-eval=fp ...

(cpp/src/vs.cc:107-408), one game per CPU thread.  This plays the same matches as batches of whole games resident on the GPU, both seats
searching on the forest search (oak_amd.arena.search_match), and prints the reference's report.

usage: search_match.py [--budget N] [--bandit ucb-2.0] [--eval mc|fp|FILE.battle.net] [--policy-mode e] [--policy-temp T] [--policy-min M]
                       [--pX-budget ... --pX-bandit ... --pX-eval ... --pX-policy-mode ... --pX-policy-temp ... --pX-policy-min ...
                        --pX-discrete]   (X = 1, 2: that seat alone; the unprefixed flags set both)
                       [--max-games N] [--teams FILE] [--mirror-match] [--early-stop 10.0] [--max-turns 1000] [--no-nash | --device-nash] [--seed S]
                       [--json out.json] [--dir DIR]

--budget: iterations (time budgets are not run by the forest search).  --bandit: ucb-<c> or pucb-<c> (pucb needs a network eval).
--max-games N: matches, as vs counts them: two teams are drawn per match and played in both seatings with the agents swapped, so 2 N games
-- N with --mirror-match, where both sides get the same team.  --teams FILE: JSON {"teams": [[[species, move x 4] x 6] ...]} by name (the
default: the reference's 16 sample teams).  --early-stop: vs's threshold (0 = off).  Output: `score: ... over ... games; Elo diff: ...`,
`W D L:` and the three counts from agent 1's point of view, then the early stops and the games cut at --max-turns.
--dir DIR: every game is also saved as vs saves it (vs.cc:380-395), one record per seat: DIR/p1/<k>.battle.data and DIR/p2/<k>.battle.data per
seating k (in seating 1 the agents are swapped: seat p1 is agent 2); the paths are printed.  A seat with one choice is not searched: its
update has iterations 0, which a loader's min_iterations skips.  tools/verify_battle_data.py DIR/p1 DIR/p2 replays them."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIELDS = (("budget", int, 1024), ("bandit", str, "ucb-2.0"), ("eval", str, "mc"), ("policy_mode", str, "e"), ("policy_temp", float, 1.0),
          ("policy_min", float, 0.0))


def agent(a, seat):
    """The seat's agent dict for arena.search_match from the --pX-* flags, falling back to the unprefixed ones."""
    get = lambda name: getattr(a, "p%d_%s" % (seat, name)) if getattr(a, "p%d_%s" % (seat, name)) is not None else getattr(a, name)
    kind, _, c = get("bandit").partition("-")
    if kind not in ("ucb", "pucb"):
        raise SystemExit("search_match: the forest search runs ucb-<c> and pucb-<c> (got %r)" % get("bandit"))
    ev = {"mc": "mc", "": "mc", "fp": "poke-engine"}.get(get("eval"), get("eval"))
    return dict(iterations=get("budget"), bandit=kind, c=float(c or 2.0), evaluator=ev, discrete=getattr(a, "p%d_discrete" % seat),
                policy_mode=get("policy_mode"), policy_temp=get("policy_temp"), policy_min=get("policy_min"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name, kind, default in FIELDS:
        ap.add_argument("--" + name.replace("_", "-"), type=kind, default=default)
        for seat in (1, 2):
            ap.add_argument("--p%d-%s" % (seat, name.replace("_", "-")), type=kind, default=None)
    ap.add_argument("--p1-discrete", action="store_true")
    ap.add_argument("--p2-discrete", action="store_true")
    ap.add_argument("--max-games", type=int, default=1024)
    ap.add_argument("--teams", default=os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json"))
    ap.add_argument("--mirror-match", action="store_true")
    ap.add_argument("--early-stop", type=float, default=10.0)
    ap.add_argument("--max-turns", type=int, default=1000)
    ap.add_argument("--no-nash", action="store_true")
    ap.add_argument("--device-nash", action="store_true", help="solve the root matrices on the GPU (the same bits, no host round trip)")
    ap.add_argument("--seed", type=int, default=0x0A4B)
    ap.add_argument("--json")
    ap.add_argument("--dir")
    a = ap.parse_args()
    a1, a2 = agent(a, 1), agent(a, 2)
    import torch
    torch.cuda.init()   # torch initialises the GPU before the library does
    from oak_amd import arena
    from oak_amd.engine import Context
    from policy_match import team_bytes
    ctx = Context(0)
    res = arena.search_match(ctx, a1, a2, team_bytes(a.teams), a.max_games, a.seed, mirror=a.mirror_match, max_turns=a.max_turns, early_stop=a.early_stop,
                             solve_nash=False if a.no_nash else ("device" if a.device_nash else True), records_dir=a.dir)
    print("score: %g over %d games; Elo diff: %g" % (res["score"], res["games"], res["elo"]))
    print("W D L:")
    print("%d %d %d" % (res["W"], res["D"], res["L"]))
    print("early stops: %d; stopped at %d turns: %d; zero policies: %d" % (res["early_stops"], a.max_turns, res["stopped"], res["zero_policy"]))
    for path in res.get("record_files", []):
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(res, p1=a1, p2=a2, matches=a.max_games, mirror=a.mirror_match, early_stop=a.early_stop, max_turns=a.max_turns, seed=a.seed), f)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
