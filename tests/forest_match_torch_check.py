"""Child process of tests/test_gpu_forest_match.py: search_games on torch tensors (torch initialises the GPU first).  Device tensors in give
device tensors out, equal to the host-array call's byte for byte.  Prints "forest match torch ok"."""
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
    from oak_amd.arena import search_games
    from oak_amd.engine import Context
    from oak_amd.search import Forest
    from test_oracle_goldens import benchmark_teams
    n, log_turns = 9, 400
    teams = np.stack([np.array(benchmark_teams(), dtype=np.uint8).reshape(60)] * n)
    battle_seeds = np.arange(n, dtype=np.uint64) + np.uint64(41000)
    seeds = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(5)
    ctx = Context(0)
    b, d, r = ctx.battle(teams, battle_seeds)
    seats = (dict(iterations=8, bandit="ucb", c=2.0, evaluator="poke-engine", policy_mode="e0.5-n0.5"), dict(iterations=4, bandit="ucb", c=2.0, evaluator="mc"))
    kw = dict(log_turns=log_turns, early_stop=10.0)
    want = search_games(ctx, seats, b, d, r, seeds, **kw)
    tb, td, tr = (torch.from_numpy(x).to(dev) for x in (b, d, r))
    ts = torch.from_numpy(seeds.view(np.int64)).to(dev)
    forest = Forest(ctx, 12, 10)
    for _ in range(2):   # the second call reuses the forest and its workspace
        got = search_games(ctx, seats, tb, td, tr, ts, forest=forest, **kw)
        assert all(got[k].is_cuda for k in ("results", "turns", "status", "log"))
        torch.cuda.synchronize()
        for k in ("results", "turns", "status", "log"):
            assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        assert got["counts"] == want["counts"] and sum(got["counts"]) == n
    forest.close()
    ctx.close()
    print("forest match torch ok")


if __name__ == "__main__":
    main()
