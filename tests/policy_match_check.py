"""Child process of tests/test_gpu_policy_games.py (torch initialises the GPU first): arena.match over 16 team pairs -- both seatings
accounted from net A's side against a count by hand from the games' result bytes, the same seed giving the same triple, mirror playing
one seating of one team per side -- and arena.policy_games on torch tensors against its host-array form, bit for bit.  Prints
"policy match ok"."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    import oracle_lib as O
    from oak_amd import arena, gamedata as G
    from oak_amd.engine import Context, Network
    ctx = Context(0)
    tiny = Network(ctx, path=os.path.join(ROOT, "tests", "golden", "net_tiny.battle.net"))
    teams = json.load(open(os.path.join(ROOT, "tests", "golden", "ou_sample_teams.json")))["teams"]
    tb = np.array([[[G.match_species(s[0])] + [G.match_move(m) for m in s[1:]] for s in t] for t in teams], dtype=np.uint8)
    res = arena.match(ctx, tiny, tiny, tb, 16, seed=11, return_games=True)
    assert res["W"] + res["D"] + res["L"] == 32 == res["games"] and len(res["seatings"]) == 2
    w = d = l = 0
    for k, s in enumerate(res["seatings"]):
        t = s["results"] & 15
        assert len(t) == 16 and s["a_is_p1"] == (k == 0) and ((t >= 1) & (t <= 3) | (s["turns"] == 1000)).all()
        wins, losses = int((t == 1).sum()), int((t == 2).sum())
        w += wins if s["a_is_p1"] else losses          # the second seating is flipped: B sat in seat p1
        l += losses if s["a_is_p1"] else wins
        d += int(((t == 3) | (t == 0)).sum())
    assert (res["W"], res["D"], res["L"]) == (w, d, l), (res, w, d, l)
    assert abs(res["score"] - (w + 0.5 * d) / 32) < 1e-15
    if 0 < res["score"] < 1:
        assert abs(res["elo"] - (np.log(res["score"]) - np.log(1 - res["score"])) * 400 / np.log(10)) < 1e-9
    assert (res["seatings"][0]["teams"] == res["seatings"][1]["teams"]).all() and (res["seatings"][0]["battle_seeds"] != res["seatings"][1]["battle_seeds"]).any()
    again = arena.match(ctx, tiny, tiny, tb, 16, seed=11)
    assert (again["W"], again["D"], again["L"]) == (w, d, l)
    by_path = arena.match(ctx, os.path.join(ROOT, "tests", "golden", "net_tiny.battle.net"), None, tb, 16, seed=11, mirror=True, return_games=True)
    assert by_path["games"] == 16 and len(by_path["seatings"]) == 1
    picked = by_path["seatings"][0]["teams"]
    assert (picked[:, 0] == picked[:, 1]).all()
    # torch tensors in, torch tensors out: the host-array form's bytes
    b, dd, p, r = O.make_random_ou_batch(200, seed0=0x5EA7)
    host = arena.policy_games(ctx, (tiny, None), b, dd, r, p, log_turns=40, return_state=True)
    t = lambda x: torch.from_numpy(x).to(dev)
    gpu = arena.policy_games(ctx, (tiny, None), t(b), t(dd), t(r), t(p), log_turns=40, return_state=True)
    torch.cuda.synchronize()
    for k in ("results", "turns", "values", "prng", "battles", "durations", "log"):
        assert gpu[k].is_cuda and gpu[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    assert gpu["counts"] == host["counts"] and sum(host["counts"]) == 200
    print("policy match ok")


if __name__ == "__main__":
    main()
