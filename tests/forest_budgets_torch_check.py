"""Child process of tests/test_gpu_forest_budgets.py: forest_search with budgets on torch tensors (torch initialises the GPU first).  Device
tensors in give device tensors out, equal to the host-array call's numbers and trace byte for byte.  Prints "forest budgets torch ok"."""
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
    from oak_amd.search import Forest, forest_search
    from test_gpu_forest_budgets import ITER, budgets_for
    from test_gpu_search_forest import roots
    b, d, r, seeds, twin = roots(33)
    bud = budgets_for(33, "random")
    ctx = Context(0)
    want = forest_search(ctx, b, d, r, seeds, ITER, c=1.0, evaluator="poke-engine", trace_levels=100, budgets=bud)
    tb, td, tr = (torch.from_numpy(x).to(dev) for x in (b, d, r))
    ts = torch.from_numpy(seeds.view(np.int64)).to(dev)
    tbud = torch.from_numpy(bud.astype(np.int32)).to(dev)
    forest = Forest(ctx, 40, 30)
    got = forest_search(ctx, tb, td, tr, ts, ITER, c=1.0, evaluator="poke-engine", trace_levels=100, forest=forest, budgets=tbud)
    assert all(v.is_cuda for v in got.values())
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in got.items()}
    for g in range(33):
        w = want[g]
        m, n = w["m"], w["n"]
        assert host["iterations"][g] == bud[g] and host["nodes"][g] == w["nodes"], g
        assert (host["visit_matrix"][g][:m, :n] == w["visit_matrix"]).all() and host["value_matrix"][g][:m, :n].tobytes() == w["value_matrix"].tobytes(), g
        assert host["total_depth"][g] == w["raw"].total_depth and int(host["stream"][g:g + 1].view(np.uint64)[0]) == w["stream"], g
        assert host["trace"][g].tobytes() == w["trace"].tobytes(), g
    assert forest.last_rows()[1] == int(bud.sum())
    forest.close()
    ctx.close()
    print("forest budgets torch ok")


if __name__ == "__main__":
    main()
