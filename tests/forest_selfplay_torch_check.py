"""Child process of tests/test_gpu_forest_selfplay.py: forest_selfplay on torch tensors (torch initialises the GPU first).  Device tensors in
give device tensors out, equal to the host-array call's byte for byte.  Prints "forest selfplay torch ok"."""
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
    from oak_amd.engine import Context
    from oak_amd.frames import forest_selfplay
    from oak_amd.search import Forest
    from test_oracle_goldens import benchmark_teams
    n, iterations = 9, 8
    teams = np.stack([np.array(benchmark_teams(), dtype=np.uint8).reshape(60)] * n)
    battle_seeds = np.arange(n, dtype=np.uint64) + np.uint64(31000)
    seeds = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(5)
    ctx = Context(0)
    kw = dict(c=2.0, evaluator="poke-engine", policy_mode="e0.5-n0.5")
    want = forest_selfplay(ctx, teams, battle_seeds, seeds, iterations, **kw)
    tt = torch.from_numpy(teams).to(dev)
    tb, ts = (torch.from_numpy(x.view(np.int64)).to(dev) for x in (battle_seeds, seeds))
    forest = Forest(ctx, 12, 10)
    for _ in range(2):   # the second call reuses the forest and its workspace
        got = forest_selfplay(ctx, tt, tb, ts, iterations, forest=forest, **kw)
        assert all(v.is_cuda for v in got)
        torch.cuda.synchronize()
        stream, offsets, n_frames, results, status = (v.cpu().numpy() for v in got)
        assert stream.tobytes() == want[0] and (offsets.view(np.uint64) == want[1]).all()
        assert (n_frames.view(np.uint32) == want[2]).all() and (results == want[3]).all() and (status == want[4]).all() and (status == 0).all()
    forest.close()
    ctx.close()
    print("forest selfplay torch ok")


if __name__ == "__main__":
    main()
