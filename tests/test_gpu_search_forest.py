"""GPU: the forest search (oak_amd/csrc/forest.hip; contract in include/oakgpu.h) -- n searches at once, one lane per tree.
  1. UCB trees equal tree_search(batch=1, seed=seeds[g]) bit for bit: every output field but the duration, node count, total depth,
     the root bandits and the continuing fast_prng stream, for every evaluator;
  2. PUCB trees are held to their own traces by tests/forest_ref.py's replayer, root priors / logits to the host search's;
  3. a tree's bytes do not depend on the rows beside it, on the forest's capacity or on what the forest ran before;
  4. iterations = max_iterations fills the arena without the error word;
  5. the C++, pyoak and torch faces return the C call's numbers."""
import os
import subprocess

import numpy as np
import pytest

import forest_ref as R
from oak_amd.parse import parse_battle, result_from_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# search-test.cc's family (1 hp on both sides, a single legal action on one side or both) and two positions whose only moves fail at
# full hp: a one-action chain that every iteration walks one level deeper
PLANTED = ("starmie seismictoss 1hp (conf:3) | snorlax bodyslam 1hp", "starmie seismictoss 1hp slp6 | snorlax seismictoss 1hp",
           "starmie seismictoss 101hp slp3 | snorlax seismictoss 1hp", "starmie surf recover 1hp | rhydon earthquake 1hp",
           "chansey softboiled | snorlax rest", "chansey softboiled | chansey softboiled",
           "chansey softboiled seismictoss | snorlax rest bodyslam")
FIELDS = ("m", "n", "p1_choices", "p2_choices", "visit_matrix", "value_matrix", "iterations", "initial_value", "nodes", "mean_depth", "nash_value",
          "p1_nash", "p2_nash", "empirical_value", "p1_empirical", "p2_empirical", "p1_logit", "p2_logit", "p1_prior", "p2_prior")
_CACHE = {}


def roots(n):
    """n non-terminal roots: mid-game random-OU states (thirds advanced 8 / 20 / 35 turn-steps), the PLANTED end-games at rows 3, 7, 11, ..., and row 70 (or the last row) a copy of row 0, seed included."""
    if n in _CACHE:
        return _CACHE[n]
    import oracle_lib as O
    b, d, p, r = O.make_random_ou_batch(2 * n, seed0=0xF0E57)
    parts = np.array_split(np.arange(2 * n), 3)
    for k, idx in zip((8, 20, 35), parts):
        bb, dd, pp, rr = (np.ascontiguousarray(x[idx]) for x in (b, d, p, r))
        out, _ = O.rollout_batch(bb, dd, rr, pp, max_steps=k, threads=4)
        b[idx], d[idx], r[idx] = bb, dd, out
    live = np.flatnonzero((r & 15) == 0)[::2][:n]           # every other one: all three thirds are present
    assert len(live) == n
    b, d, r = b[live].copy(), d[live].copy(), r[live].copy()
    for q, text in enumerate(PLANTED):
        row = 3 + 4 * q
        if row < n:
            pb, pd = parse_battle(text)
            b[row], d[row], r[row] = pb, pd, result_from_state(pb)
    seeds = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345)).astype(np.uint64)
    twin = 70 if n > 70 else n - 1
    b[twin], d[twin], r[twin], seeds[twin] = b[0], d[0], r[0], seeds[0]
    _CACHE[n] = (b, d, r, seeds, twin)
    return _CACHE[n]


def network(ctx, tmp_path, name):
    from oak_amd.engine import Network
    import policy_ref as P
    if name == "default_int8":   # the quantized handle (net_tiny's widths are not among the quantized network's: its loader refuses it)
        return Network(ctx, path=P.rewrite_net(P.GOLDEN["default"], str(tmp_path / "default_int8.battle.net"), P.spread_main_net, header0=1), discrete=True)
    return Network(ctx, path=P.GOLDEN[name])


def same_output(a, b):
    for f in FIELDS:
        x, y = np.asarray(a[f]), np.asarray(b[f])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (f, a[f], b[f])


def coverage(trees, max_depth):
    got = {"terminal": 0, "deep": 0, "k1": 0, "capped": 0}
    cap = max_depth if max_depth else 100
    for t in trees:
        tr = t["trace"]
        got["terminal"] += int((tr["result_type"] != 0).sum())
        got["deep"] += int((tr["levels"] >= 3).sum())
        got["capped"] += int(((tr["leaf"] != R.NO_NODE) & (tr["initialised"] == 0) & (tr["levels"] == cap)).sum())
        got["k1"] += sum(1 for p1, p2 in t["tree"] if p1[0] == 1 or p2[0] == 1)
    return got


# ---- 1. UCB: the host search, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("evaluator, n, iterations, max_depth", [("poke-engine", 96, 48, 0), ("mc", 33, 24, 0), ("tiny", 33, 24, 0), ("default_int8", 33, 24, 0),
                                                                 ("poke-engine", 96, 48, 3), ("mc", 33, 24, 3)])
def test_ucb_trees_equal_the_host_search(gpu_ctx, tmp_path, evaluator, n, iterations, max_depth):
    from oak_amd.search import Heap, forest_search, search_stream, tree_search
    b, d, r, seeds, twin = roots(n)
    ev = evaluator if evaluator in ("mc", "poke-engine") else network(gpu_ctx, tmp_path, evaluator)
    trees = forest_search(gpu_ctx, b, d, r, seeds, iterations, c=1.0, evaluator=ev, max_depth=max_depth, solve_nash=True,
                          trace_levels=max_depth if max_depth else 100)
    if (evaluator, max_depth) == ("poke-engine", 0):
        _CACHE["reference trees"] = trees
    cover = coverage(trees, max_depth)
    print("coverage", evaluator, n, iterations, max_depth, cover)
    assert cover["terminal"] and cover["deep"] and cover["k1"], cover
    if max_depth:
        assert cover["capped"], cover
    heap = Heap()
    for g in range(n):
        heap.clear()
        want = tree_search(gpu_ctx, b[g], d[g], int(r[g]), iterations=iterations, batch=1, c=1.0, evaluator=ev, max_depth=max_depth if max_depth else 100,
                           seed=int(seeds[g]), heap=heap)
        same_output(trees[g], want)
        assert trees[g]["raw"].total_depth == want["raw"].total_depth and trees[g]["stream"] == search_stream(gpu_ctx), g
        for player in (0, 1):
            sc, pr, vi = heap.root_stats(player)
            k, fs, fp, fv = trees[g]["tree"][0][player]
            assert k == len(sc) and fs[:k].tobytes() == sc.tobytes() and fp[:k].tobytes() == pr.tobytes() and fv[:k].tobytes() == vi.tobytes(), (g, player)
        assert int(trees[g]["visit_matrix"].sum()) == iterations and len(trees[g]["tree"]) == trees[g]["nodes"]
        R.replay(trees[g]["trace"], trees[g]["tree"], R.UCB, 1.0, max_depth)
    same_output(trees[0], trees[twin])
    assert trees[0]["stream"] == trees[twin]["stream"] and trees[0]["trace"].tobytes() == trees[twin]["trace"].tobytes()
    heap.close()
    if not isinstance(ev, str):
        ev.close()


# ---- 2. PUCB: held to its own trace ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "default"])
def test_pucb_trees_follow_their_traces(gpu_ctx, tmp_path, name):
    from oak_amd.search import forest_search, tree_search
    n, iterations = 65, 32
    b, d, r, seeds, twin = roots(n)
    net = network(gpu_ctx, tmp_path, name)
    trees = forest_search(gpu_ctx, b, d, r, seeds, iterations, c=1.0, bandit="pucb", evaluator=net, trace_levels=100)
    worst = 0.0
    for g in range(n):
        t = trees[g]
        m, nn = t["m"], t["n"]
        R.replay(t["trace"], t["tree"], R.PUCB, 1.0, 0, (t["p1_logit"], t["p2_logit"]))
        host = tree_search(gpu_ctx, b[g], d[g], int(r[g]), iterations=0, batch=1, c=1.0, bandit="pucb", evaluator=net, seed=int(seeds[g]))
        assert t["p1_logit"].tobytes() == host["p1_logit"].tobytes() and t["p2_logit"].tobytes() == host["p2_logit"].tobytes(), g
        assert t["initial_value"] == host["initial_value"] and int(t["visit_matrix"].sum()) == iterations
        for mine, theirs, k, node in ((t["p1_prior"], host["p1_prior"], m, t["tree"][0][0]), (t["p2_prior"], host["p2_prior"], nn, t["tree"][0][1])):
            err = float(np.max(np.abs(mine[:k] - theirs[:k]) / theirs[:k]))
            worst = max(worst, err)
            assert err <= R.PRIOR_BOUND, (g, err)
            assert np.max(np.abs(node[2][:k].astype(np.float64) - theirs[:k]) / theirs[:k]) <= R.PRIOR_BOUND, g
    print("pucb", name, "worst root prior error vs the host search: %.3g (bound %.3g)" % (worst, R.PRIOR_BOUND))
    same_output(trees[0], trees[twin])
    net.close()


# ---- 3. independence ---------------------------------------------------------------------------------------------------------------
def tree_bytes(t):
    return b"".join(np.asarray(t[f]).tobytes() for f in FIELDS) + t["trace"].tobytes() + np.uint64(t["stream"]).tobytes() + \
        b"".join(np.asarray(x).tobytes() for node in t["tree"] for side in node for x in side[1:])


def test_a_tree_does_not_depend_on_its_neighbours_or_the_forest(gpu_ctx):
    from oak_amd.search import Forest, forest_search
    b, d, r, seeds, twin = roots(96)
    iterations = 48
    ref = _CACHE.get("reference trees") or forest_search(gpu_ctx, b, d, r, seeds, iterations, c=1.0, evaluator="poke-engine", solve_nash=True, trace_levels=100)
    want = [tree_bytes(t) for t in ref]
    rng = np.random.default_rng(5)
    big = Forest(gpu_ctx, 200, 77)
    for count, forest in ((1, None), (63, None), (64, big), (65, big), (1, big)):
        rows = rng.permutation(96)[:count]
        got = forest_search(gpu_ctx, b[rows], d[rows], r[rows], seeds[rows], iterations, c=1.0, evaluator="poke-engine", solve_nash=True, trace_levels=100,
                            forest=forest)
        for q, g in enumerate(rows):
            if forest is not None:
                got[q]["tree"] = forest.nodes(q)
            assert tree_bytes(got[q]) == want[g], (count, q, g)
    big.close()


# ---- 4. capacity -------------------------------------------------------------------------------------------------------------------
def test_a_full_arena_is_not_an_overflow(gpu_ctx):
    from oak_amd.search import Forest, forest_search
    b, d, r, seeds, twin = roots(33)
    forest = Forest(gpu_ctx, 33, 24)
    got = forest_search(gpu_ctx, b, d, r, seeds, 24, c=1.0, evaluator="mc", forest=forest)      # raises on the error word
    nodes = np.array([t["nodes"] for t in got])
    print("nodes per tree", nodes.tolist())
    # every iteration that does not end on a terminal edge creates a node: the mid-game trees hold 1 + 24 nodes, their arenas exactly full
    assert nodes.max() == 25 and (nodes == 25).sum() >= 8 and (nodes >= 1).all()
    again = forest_search(gpu_ctx, b, d, r, seeds, 24, c=1.0, evaluator="mc", forest=forest)    # the same object, a second call
    for x, y in zip(got, again):
        same_output(x, y)
    stats = forest.last_stats()
    assert stats[0] == 24 and stats[1] >= 24 and stats[3] <= stats[1]
    forest.close()


# ---- 5. faces ----------------------------------------------------------------------------------------------------------------------
def test_cpp_face_equals_the_c_call_and_the_host_search(tmp_path):
    exe = str(tmp_path / "cpp_forest_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_forest_smoke.cc"), "-L",
                           os.path.join(ROOT, "oak_amd"), "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "forest == c call == tree search" in out.stdout and out.stdout.strip().endswith("ok"), out.stdout


def test_torch_face_in_a_child_process():
    """forest_search with torch tensors on the device, through tests/forest_torch_check.py in a child process -- torch must initialise the
    GPU before the library does."""
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "forest_torch_check.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "forest torch ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_pyoak_face_equals_the_c_call(gpu_ctx):
    from oak_amd import pyoak
    from oak_amd.search import forest_search
    b, d, r, seeds, twin = roots(33)
    iterations = 24
    want = forest_search(gpu_ctx, b, d, r, seeds, iterations, c=1.0, evaluator="poke-engine", solve_nash=True)
    agent = pyoak.Agent()
    agent.budget, agent.bandit, agent.eval = str(iterations), "ucb-1.0", "fp"
    outs = pyoak.search_forest(b, d, r, seeds, agent)
    assert len(outs) == 33
    for g in range(33):
        w, o = want[g], outs[g]
        m, n = w["m"], w["n"]
        assert o.m == m and o.n == n and o.iterations == iterations and o.empirical_value == w["empirical_value"] and o.nash_value == w["nash_value"]
        assert (o.visit_matrix[:m, :n] == w["visit_matrix"]).all() and o.value_matrix[:m, :n].tobytes() == w["value_matrix"].tobytes()
        assert o.p1_nash[:m].tobytes() == w["p1_nash"].tobytes() and o.p2_empirical[:n].tobytes() == w["p2_empirical"].tobytes()
    for text, fields in (("time budgets", dict(budget="10ms")), ("matrix_ucb", dict(matrix_ucb="16-16-2-1.0")), ("Exp3", dict(bandit="exp3-0.1"))):
        bad = pyoak.Agent()
        bad.budget, bad.bandit, bad.eval = str(iterations), "ucb-1.0", "mc"
        for k, v in fields.items():
            setattr(bad, k, v)
        with pytest.raises(RuntimeError, match=text):
            pyoak.search_forest(b, d, r, seeds, bad)
