"""GPU: per-tree budgets in the forest search (oakgpu_forest_search_budgets*; contract in include/oakgpu.h).
  1. tree g of a budgets call equals, byte for byte, tree g of the call without budgets at iterations = budgets[g]: every output array, every
     node, the trace records below the budget; records past it, and guard bands round every array, keep their fill -- UCB and PUCB, the three
     evaluators, a depth cap, three row orders, 33 / 65 / 130 trees;
  2. the same on a kept forest across an advance;
  3. the accounting: launched == run for non-increasing budgets, launched == n * max for non-decreasing ones;
  4. a tree does not depend on its neighbours' budgets;
  5. the C++, pyoak and torch faces equal the C call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_search_forest import FIELDS, network, roots, same_output, tree_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGETS, ITER = (1, 7, 24), 24
GUARD = 64


def budgets_for(n, order):
    b = np.random.default_rng(1000 + n).choice(np.array(BUDGETS, np.uint32), size=n)
    b[:3] = BUDGETS   # every budget is present
    if order == "non-increasing":
        b = np.sort(b)[::-1]
    elif order == "non-decreasing":
        b = np.sort(b)
    return np.ascontiguousarray(b, dtype=np.uint32)


def params(iterations, bandit, use_net, evaluator, max_depth):
    from oak_amd import _lib
    return _lib.SearchParams(iterations=int(iterations), batch=1, ucb_c=1.0, bandit={"ucb": 0, "pucb": 1}[bandit],
                             eval=1 if use_net else {"mc": 0, "poke-engine": 2}[evaluator], max_depth=int(max_depth), root_rolls=3, other_rolls=1, seed=0,
                             matrix_ucb=0, mucb_delay=0, mucb_minimum=0, mucb_c=0.0, exp3_alpha=-1.0, duration_us=0)


def dev_search(ctx, forest, b, d, r, seeds, iterations, budgets=None, bandit="ucb", evaluator="poke-engine", max_depth=0, keep=False, trace_levels=100):
    """The device-array call on raw buffers: every output array and the trace sit in allocations filled with 0xFF (a NaN in the doubles), GUARD bytes
    round each.  Returns ({field: array [n, ...]}, trace uint8 [n, iterations, record], [node bytes per tree]); asserts the guards are untouched."""
    from hipmem import Dev
    from oak_amd import _lib
    from oak_amd.search import _FOREST_TENSORS
    n = len(r)
    use_net = not isinstance(evaluator, str)
    prm = params(iterations, bandit, use_net, evaluator, max_depth)
    ins = [Dev(np.ascontiguousarray(b)), Dev(np.ascontiguousarray(d)), Dev(np.ascontiguousarray(r)), Dev(np.ascontiguousarray(seeds, dtype=np.uint64))]
    db = Dev(np.ascontiguousarray(budgets, dtype=np.uint32)) if budgets is not None else None
    outs = {}
    for name, dt, tail in _FOREST_TENSORS:
        host = np.zeros((n,) + tail, dtype=np.dtype(dt))
        outs[name] = (Dev(np.zeros(host.nbytes + 2 * GUARD, np.uint8), fill=0xFF), host)
    ptrs = _lib.ForestOutputs(**{name: outs[name][0].p.value + GUARD for name, _, _ in _FOREST_TENSORS})
    rec = C.sizeof(_lib.ForestTraceHead) + trace_levels * C.sizeof(_lib.ForestTraceLevel)
    trace = Dev(np.zeros(n * iterations * rec + 2 * GUARD, np.uint8), fill=0xFF)
    lib = ctx.lib
    head = (forest.handle, use_net and evaluator.handle or None, C.byref(prm), ins[0].p, ins[1].p, ins[2].p, ins[3].p)
    tail = (n, C.byref(ptrs), C.c_void_p(trace.p.value + GUARD), trace_levels)
    if budgets is None:
        _lib.check((lib.oakgpu_forest_search_kept_dev if keep else lib.oakgpu_forest_search_dev)(*head, *tail))
    else:
        _lib.check((lib.oakgpu_forest_search_budgets_kept_dev if keep else lib.oakgpu_forest_search_budgets_dev)(*head, db.p, *tail))
    got = {}
    for name, (dev, host) in outs.items():
        raw = dev.host()
        assert (raw[:GUARD] == 0xFF).all() and (raw[-GUARD:] == 0xFF).all(), name
        got[name] = raw[GUARD:-GUARD].view(host.dtype).reshape(host.shape)
    raw = trace.host()
    assert (raw[:GUARD] == 0xFF).all() and (raw[-GUARD:] == 0xFF).all()
    tr = raw[GUARD:-GUARD].reshape(n, iterations, rec)
    nodes = []
    for g in range(n):
        count = int(got["nodes"][g])
        buf = (_lib.ForestNode * max(count, 1))()
        _lib.check(lib.oakgpu_forest_nodes(forest.handle, g, 0, count, buf))
        nodes.append(bytes(buf)[:count * C.sizeof(_lib.ForestNode)])
    for x in ins + [trace] + [v[0] for v in outs.values()] + ([db] if db else []):
        x.free()
    return got, tr, nodes


def assert_tree_equals(got, want, g, budget, q=None):
    """tree g of a budgets call against tree q (default g) of the uniform call with iterations = budget"""
    q = g if q is None else q
    (go, gt, gn), (wo, wt, wn) = got, want
    for name in go:
        assert go[name][g].tobytes() == wo[name][q].tobytes(), (name, g, budget)
    assert int(go["iterations"][g]) == budget
    assert gt[g, :budget].tobytes() == wt[q, :budget].tobytes(), ("trace", g, budget)
    assert (gt[g, budget:] == 0xFF).all(), ("records past the budget", g, budget)
    assert gn[g] == wn[q], ("nodes", g, budget)


CONFIGS = {"ucb-pe": ("ucb", "poke-engine", 0), "ucb-mc": ("ucb", "mc", 0), "ucb-tiny": ("ucb", "tiny", 0), "pucb-tiny": ("pucb", "tiny", 0),
           "ucb-pe-depth2": ("ucb", "poke-engine", 2)}


# ---- 1. equality with the uniform calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 65, 130])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_a_budgets_tree_is_the_uniform_calls_tree(gpu_ctx, tmp_path, config, n):
    from oak_amd.search import Forest
    bandit, evaluator, max_depth = CONFIGS[config]
    b, d, r, seeds, twin = roots(n)
    ev = evaluator if evaluator in ("mc", "poke-engine") else network(gpu_ctx, tmp_path, evaluator)
    forest = Forest(gpu_ctx, n, ITER, contextual=bandit == "pucb")
    kw = dict(bandit=bandit, evaluator=ev, max_depth=max_depth, trace_levels=max_depth if max_depth else 100)
    want = {k: dev_search(gpu_ctx, forest, b, d, r, seeds, k, **kw) for k in BUDGETS}
    for k in BUDGETS:   # (the uniform call itself: every record written, the accounting n * iterations)
        assert (want[k][0]["iterations"] == k).all()
    assert forest.last_rows() == (n * ITER, n * ITER)
    for order in ("random", "non-increasing", "non-decreasing"):
        budgets = budgets_for(n, order)
        got = dev_search(gpu_ctx, forest, b, d, r, seeds, ITER, budgets=budgets, **kw)
        for g in range(n):
            assert_tree_equals(got, want[int(budgets[g])], g, int(budgets[g]))
        launched, run = forest.last_rows()
        assert run == int(budgets.sum()) and launched >= run
        if order == "non-increasing":
            assert launched == run
        if order == "non-decreasing":
            assert launched == n * ITER
    forest.close()
    if not isinstance(ev, str):
        ev.close()


# ---- 2. kept forests ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("evaluator", ["poke-engine", "mc"])
def test_budgets_on_a_kept_forest_across_an_advance(gpu_ctx, evaluator):
    from oak_amd.search import Forest, forest_search
    from test_gpu_forest_keep import play
    n = 33
    b, d, r, seeds, twin = roots(n)
    first = budgets_for(n, "random")
    then = {1: 24, 7: 1, 24: 7}
    second = np.array([then[int(x)] for x in first], np.uint32)
    forest = Forest(gpu_ctx, n, ITER, keep_arena=0)

    def two_calls(rows, bud1, bud2):
        """search, play the most visited cell, advance the rows that go on, search again: (first outputs, rows that went on, second outputs + nodes)"""
        bb, dd = b[rows].copy(), d[rows].copy()
        kw = dict(c=1.0, evaluator=evaluator, trace_levels=100, forest=forest)
        if np.isscalar(bud1):
            one = forest_search(gpu_ctx, bb, dd, r[rows], seeds[rows], bud1, **kw)      # (a fresh stamp: the trees of the call before are gone)
        else:
            one = forest_search(gpu_ctx, bb, dd, r[rows], seeds[rows], ITER, budgets=bud1, **kw)
        i, j, obs, res = play(gpu_ctx, one, bb, dd)
        src = np.flatnonzero((res & 15) == 0).astype(np.uint32)
        kept = forest.advance(i[src], j[src], obs[src], src=src)
        s2 = seeds[rows][src] ^ np.uint64(0xABCDEF)
        if np.isscalar(bud2):
            two = forest_search(gpu_ctx, bb[src], dd[src], res[src], s2, bud2, keep=True, **kw)
        else:
            two = forest_search(gpu_ctx, bb[src], dd[src], res[src], s2, ITER, budgets=bud2[src], keep=True, **kw)
        for q in range(len(src)):
            two[q]["tree"] = forest.nodes(q)
        return one, src, kept, two

    all_rows = np.arange(n)
    one, src, kept, two = two_calls(all_rows, first, second)
    assert kept.sum() > 0 and len(src) > n // 2
    assert forest.last_rows()[1] == int(second[src].sum())
    checked = 0
    for a in BUDGETS:
        rows = np.flatnonzero(first == a)
        w_one, w_src, w_kept, w_two = two_calls(rows, a, then[a])
        for q, g in enumerate(rows):
            same_output(one[g], w_one[q])
            assert one[g]["stream"] == w_one[q]["stream"] and one[g]["trace"][:a].tobytes() == w_one[q]["trace"].tobytes()
            assert not one[g]["trace"][a:].tobytes().strip(b"\0")
        went = {int(g): q for q, g in enumerate(src)}
        for q, local in enumerate(w_src):
            g = int(rows[local])
            mine = two[went[g]]
            assert kept[went[g]] == w_kept[q]
            assert tree_bytes({**mine, "trace": mine["trace"][:then[a]]}) == tree_bytes(w_two[q]), (g, a)
            checked += 1
    assert checked == len(src)
    forest.close()


# ---- 3. refusals reach the device call ----------------------------------------------------------------------------------------------
def test_bad_budgets_are_refused_by_name(gpu_ctx):
    from oak_amd._lib import OakGpuError
    from oak_amd.search import forest_search
    b, d, r, seeds, twin = roots(33)
    bud = budgets_for(33, "random")
    for at, value, text in ((5, 0, "the budget of tree 5 is 0"), (9, 25, r"the budget of tree 9 \(25\) exceeds params->iterations \(24\)")):
        bad = bud.copy()
        bad[at] = value
        bad[20] = value
        with pytest.raises(OakGpuError, match=text):
            forest_search(gpu_ctx, b, d, r, seeds, ITER, evaluator="poke-engine", budgets=bad)


# ---- 4. independence ----------------------------------------------------------------------------------------------------------------
def test_a_tree_does_not_depend_on_its_neighbours_budgets(gpu_ctx):
    from oak_amd.search import forest_search
    b, d, r, seeds, twin = roots(65)
    kw = dict(c=1.0, evaluator="mc", solve_nash=True, trace_levels=100)
    base = budgets_for(65, "random")
    ref = forest_search(gpu_ctx, b, d, r, seeds, ITER, budgets=base, **kw)
    for other in (1, 24):
        bud = np.full(65, other, np.uint32)
        bud[10], bud[64] = base[10], base[64]
        got = forest_search(gpu_ctx, b, d, r, seeds, ITER, budgets=bud, **kw)
        for g in (10, 64):
            assert tree_bytes(got[g]) == tree_bytes(ref[g]), (other, g)


# ---- 5. faces -----------------------------------------------------------------------------------------------------------------------
def test_pyoak_face_with_budgets_equals_the_c_call(gpu_ctx):
    from oak_amd import pyoak
    from oak_amd.search import forest_search
    b, d, r, seeds, twin = roots(33)
    bud = budgets_for(33, "random")
    want = forest_search(gpu_ctx, b, d, r, seeds, ITER, c=1.0, evaluator="poke-engine", solve_nash=True, budgets=bud)
    agent = pyoak.Agent()
    agent.budget, agent.bandit, agent.eval = str(ITER), "ucb-1.0", "fp"
    outs = pyoak.search_forest(b, d, r, seeds, agent, budgets=bud)
    for g in range(33):
        w, o = want[g], outs[g]
        m, n = w["m"], w["n"]
        assert o.iterations == bud[g] and o.empirical_value == w["empirical_value"] and o.nash_value == w["nash_value"]
        assert (o.visit_matrix[:m, :n] == w["visit_matrix"]).all() and o.value_matrix[:m, :n].tobytes() == w["value_matrix"].tobytes()
    bad = bud.copy()
    bad[4] = 0
    with pytest.raises(RuntimeError, match="the budget of tree 4 is 0"):
        pyoak.search_forest(b, d, r, seeds, agent, budgets=bad)


def test_cpp_face_with_budgets_equals_the_uniform_calls(tmp_path):
    exe = str(tmp_path / "cpp_forest_budgets_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_forest_budgets_smoke.cc"), "-L",
                           os.path.join(ROOT, "oak_amd"), "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_torch_face_with_budgets_in_a_child_process():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "forest_budgets_torch_check.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "forest budgets torch ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
