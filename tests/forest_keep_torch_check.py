"""Child process of tests/test_gpu_forest_keep.py: the kept forest's calls on torch tensors (torch initialises the GPU first).  Device tensors
in give device tensors out, equal to the host-array calls' values.  Prints "forest keep torch ok"."""
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
    from oak_amd.search import Forest, forest_search
    from test_oracle_goldens import benchmark_teams
    n, iterations = 9, 8
    teams = np.stack([np.array(benchmark_teams(), dtype=np.uint8).reshape(60)] * n)
    battle_seeds = np.arange(n, dtype=np.uint64) + np.uint64(32000)
    seeds = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(6)
    ctx = Context(0)
    kw = dict(c=2.0, evaluator="poke-engine", policy_mode="e0.5-n0.5", keep_node=True)
    want = forest_selfplay(ctx, teams, battle_seeds, seeds, iterations, **kw)
    tt = torch.from_numpy(teams).to(dev)
    tb, ts = (torch.from_numpy(x.view(np.int64)).to(dev) for x in (battle_seeds, seeds))
    forest = Forest(ctx, 12, 10, keep_arena=0)
    for _ in range(2):   # the second call reuses the forest, its workspace and whatever trees the first left
        got = forest_selfplay(ctx, tt, tb, ts, iterations, forest=forest, **kw)
        assert len(got) == 6 and all(v.is_cuda for v in got)
        torch.cuda.synchronize()
        stream, offsets, n_frames, results, status, nodes_kept = (v.cpu().numpy() for v in got)
        assert stream.tobytes() == want[0] and (offsets.view(np.uint64) == want[1]).all()
        assert (n_frames.view(np.uint32) == want[2]).all() and (results == want[3]).all() and (status == 0).all()
        assert (nodes_kept.view(np.uint32) == want[5]).all() and want[5].any()
    forest.close()
    # the standalone calls: a kept search, an advance with a source list, the next kept search -- tensors against host arrays
    b, d, r = ctx.battle(teams.reshape(n, 2, 6, 5), battle_seeds)
    outs = []
    for on_device in (False, True):
        forest = Forest(ctx, n, iterations, keep_arena=0)
        bb, dd = b.copy(), d.copy()
        first = forest_search(ctx, bb, dd, r, seeds, iterations, evaluator="poke-engine", forest=forest, keep=True)
        cells = [np.unravel_index(int(np.argmax(t["visit_matrix"])), t["visit_matrix"].shape) for t in first]
        i, j = np.array([c[0] for c in cells], np.uint8), np.array([c[1] for c in cells], np.uint8)
        c1 = np.array([t["p1_choices"][c[0]] for t, c in zip(first, cells)], np.uint8)
        c2 = np.array([t["p2_choices"][c[1]] for t, c in zip(first, cells)], np.uint8)
        res, obs = ctx.update(bb, c1, c2, dd)
        src = np.flatnonzero((res & 15) == 0)[::-1].copy()
        b2, d2, r2, s2 = np.ascontiguousarray(bb[src]), np.ascontiguousarray(dd[src]), np.ascontiguousarray(res[src]), seeds[src] + np.uint64(1)
        if on_device:
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            kept = forest.advance(to(i[src]), to(j[src]), to(obs[src]), src=to(src.astype(np.int32)))
            assert kept.is_cuda
            nxt = forest_search(ctx, to(b2), to(d2), to(r2), to(s2.view(np.int64)), iterations, evaluator="poke-engine", forest=forest, keep=True)
            torch.cuda.synchronize()
            outs.append((kept.cpu().numpy(), nxt["visit_matrix"].cpu().numpy(), nxt["nodes"].cpu().numpy(), nxt["stream"].cpu().numpy().view(np.uint64)))
        else:
            kept = forest.advance(i[src], j[src], obs[src], src=src)
            nxt = forest_search(ctx, b2, d2, r2, s2, iterations, evaluator="poke-engine", forest=forest, keep=True)
            vis = np.zeros((len(src), 9, 9), np.int64)
            for q, t in enumerate(nxt):
                vis[q, :t["m"], :t["n"]] = t["visit_matrix"]
            outs.append((kept, vis, np.array([t["nodes"] for t in nxt]), np.array([t["stream"] for t in nxt], np.uint64)))
        forest.close()
    assert outs[0][0].any() and all((x == y).all() for x, y in zip(outs[0], outs[1]))
    ctx.close()
    print("forest keep torch ok")


if __name__ == "__main__":
    main()
