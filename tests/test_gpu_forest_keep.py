"""GPU: kept forests (oakgpu_forest_create_kept, oakgpu_forest_advance*, oakgpu_forest_search_kept*; forest.hip) and keep_node in the game
loop over them (forestplay.hip) -- generate's --keep-node on the device.
  1. UCB trees that go on from round to round equal the host heap (tree_search(batch=1, heap) + Heap.update) bit for bit;
  2. the outcomes of an advance, planted: nothing kept / kept / a root mismatch;
  3. an advance that also moves trees between rows (a permutation, a strict subset);
  4. capacity: with keep_arena = max_iterations + 1 every subtree of two or more nodes is dropped and counted;
  5. UCB self-play with keep_node equals selfplay_game(batch=1, keep_node=True), nodes_kept included;
  6. PUCB self-play with keep_node replays, equals the standalone sequence driven here, and does not depend on the call's size;
  7. keep_node = 0 on a kept forest is the plain forest's stream; a plain forest refuses the new calls by name;
  8. the pyoak and torch faces return the C call's values."""
import os
import subprocess
import sys

import numpy as np
import pytest

import forestplay_ref as R
from oak_amd._lib import OakGpuError
from oak_amd.frames import forest_selfplay, replay_check, selfplay_game, selfplay_pick_host
from oak_amd.parse import parse_battle, result_from_state
from test_gpu_forest_selfplay import games, records
from test_gpu_search_forest import PLANTED, network, roots, same_output

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 0


def evaluator_of(ctx, tmp_path, name):
    return name if name in ("mc", "poke-engine") else network(ctx, tmp_path, name)


def most_visited(tree):
    """The most visited root cell of a search output, the lowest such cell on a tie."""
    vm = np.asarray(tree["visit_matrix"])
    i, j = np.unravel_index(int(np.argmax(vm)), vm.shape)
    return int(i), int(j)


def play(ctx, trees, b, d, cells=None):
    """One update of every row with its tree's cell (default: the most visited): (i, j, obs, results); b and d change in place."""
    cells = cells or [most_visited(t) for t in trees]
    i = np.array([c[0] for c in cells], np.uint8)
    j = np.array([c[1] for c in cells], np.uint8)
    c1 = np.array([t["p1_choices"][c[0]] for t, c in zip(trees, cells)], np.uint8)
    c2 = np.array([t["p2_choices"][c[1]] for t, c in zip(trees, cells)], np.uint8)
    res, obs = ctx.update(b, c1, c2, d)
    return i, j, obs, res


def host_search(ctx, heap, b, d, r, seed, iterations, ev, c=1.0):
    """tree_search on a heap as oakgpu_selfplay_game runs it: a root mismatch clears the heap and searches again.  Returns (output, mismatch)."""
    from oak_amd.search import tree_search
    kw = dict(iterations=iterations, batch=1, c=c, evaluator=ev, max_depth=100, seed=int(seed), heap=heap)
    try:
        return tree_search(ctx, b, d, int(r), **kw), 0
    except OakGpuError as e:
        assert "other action counts" in str(e)
        heap.clear()
        return tree_search(ctx, b, d, int(r), **kw), 1


def same_root(forest, q, heap):
    (node,) = forest.nodes(q, 0, 1)
    for player in (0, 1):
        sc, pr, vi = heap.root_stats(player)
        k, fs, fp, fv = node[player]
        assert k == len(sc) and fs[:k].tobytes() == sc.tobytes() and fp[:k].tobytes() == pr.tobytes() and fv[:k].tobytes() == vi.tobytes(), (q, player)


# ---- 1. equal to the host heap -------------------------------------------------------------------------------------------------------
def rounds_against_the_heap(ctx, ev, b, d, r, seeds, iterations, rounds=3):
    from oak_amd.search import Forest, Heap, forest_search, search_stream
    n = len(r)
    b, d, r = b.copy(), d.copy(), r.copy()
    forest = Forest(ctx, n, iterations, keep_arena=0)
    heaps = [Heap() for _ in range(n)]
    live = np.arange(n)
    kept_total = 0
    for rnd in range(rounds + 1):
        if len(live) == 0:
            break
        sd = (seeds[live] + np.uint64(1000003 * rnd)).astype(np.uint64)
        trees = forest_search(ctx, b, d, r, sd, iterations, c=1.0, evaluator=ev, solve_nash=True, forest=forest, keep=True)
        flags = forest.mismatch(len(live))
        for q, g in enumerate(live):
            want, mismatch = host_search(ctx, heaps[g], b[q], d[q], r[q], sd[q], iterations, ev)
            same_output(trees[q], want)
            assert trees[q]["raw"].total_depth == want["raw"].total_depth and trees[q]["stream"] == search_stream(ctx), (rnd, g)
            assert trees[q]["nodes"] == heaps[g].nodes() and flags[q] == mismatch, (rnd, g, trees[q]["nodes"], heaps[g].nodes(), flags[q], mismatch)
            same_root(forest, q, heaps[g])
        if rnd == rounds:
            break
        i, j, obs, res = play(ctx, trees, b, d)
        want_kept = np.array([heaps[g].update(i[q], j[q], obs[q]) for q, g in enumerate(live)], np.uint8)
        src = np.flatnonzero((res & 15) == 0)                                  # a finished position has no successor
        kept = forest.advance(i[src], j[src], obs[src], src=src)
        assert (kept == want_kept[src]).all(), (rnd, kept, want_kept[src])
        counts = forest.node_counts(len(src))
        assert all(counts[t] == (heaps[live[q]].nodes() if kept[t] else 1) for t, q in enumerate(src)), rnd
        kept_total += int(kept.sum())
        live, b, d, r = live[src], np.ascontiguousarray(b[src]), np.ascontiguousarray(d[src]), np.ascontiguousarray(res[src])
    assert forest.keep_stats()[3] == 0                                          # nothing was dropped: the comparison is the whole of it
    forest.close()
    for h in heaps:
        h.close()
    return kept_total


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("evaluator", ["poke-engine", "mc", "tiny"])
def test_kept_trees_equal_the_host_heap(gpu_ctx, tmp_path, evaluator, n):
    b, d, r, seeds, _ = roots(n)
    ev = evaluator_of(gpu_ctx, tmp_path, evaluator)
    kept = rounds_against_the_heap(gpu_ctx, ev, b, d, r, seeds, 16 if n > 1 else 32)
    print("kept", evaluator, n, kept)
    assert kept > 0 or n == 1                                                   # (one tree alone may never see its searched observation played)
    if not isinstance(ev, str):
        ev.close()


def test_kept_trees_equal_the_host_heap_int8(gpu_ctx, tmp_path):
    b, d, r, seeds, _ = roots(33)
    ev = evaluator_of(gpu_ctx, tmp_path, "default_int8")
    assert rounds_against_the_heap(gpu_ctx, ev, b, d, r, seeds, 8) > 0
    ev.close()


def test_kept_chains_longer_than_a_wave_equal_the_host_heap(gpu_ctx):
    """Positions whose only moves fail: every iteration walks one level deeper, so the kept subtree is one chain of ~150 nodes -- parents in
    earlier 64-node chunks of the advance's pass, and 63 links inside one."""
    texts = PLANTED[4:7]
    pairs = [parse_battle(t) for t in texts]
    b = np.stack([p[0] for p in pairs]).astype(np.uint8)
    d = np.stack([p[1] for p in pairs]).astype(np.uint8)
    r = np.array([result_from_state(p[0]) for p in pairs], np.uint8)
    seeds = np.array([5, 6, 7], np.uint64)
    assert rounds_against_the_heap(gpu_ctx, "poke-engine", b, d, r, seeds, 150, rounds=2) > 0


# ---- 2. the outcomes, planted ----------------------------------------------------------------------------------------------------------
def fresh(ctx, b, d, r, seeds, iterations, **kw):
    from oak_amd.search import forest_search
    return forest_search(ctx, b, d, r, seeds, iterations, solve_nash=True, **kw)


def same_tree_output(a, b):
    same_output(a, b)
    assert a["stream"] == b["stream"] and a["raw"].total_depth == b["raw"].total_depth


def test_an_unvisited_cell_keeps_nothing_and_a_visited_one_keeps_its_child(gpu_ctx, tmp_path):
    from oak_amd.search import Forest, forest_search
    n = 24
    b, d, r, seeds, _ = roots(n)
    net = network(gpu_ctx, tmp_path, "tiny")
    kw = dict(c=1.5, bandit="pucb", evaluator=net)
    for visited in (False, True):
        bb, dd = b.copy(), d.copy()
        forest = Forest(gpu_ctx, n, 8, contextual=True, keep_arena=0)
        trees = forest_search(gpu_ctx, bb, dd, r, seeds, 1, forest=forest, keep=True, solve_nash=True, **kw)   # budget 1: one cell, one child
        cells = []
        for t in trees:
            i, j = most_visited(t)
            assert int(np.asarray(t["visit_matrix"]).sum()) == 1 and t["nodes"] in (1, 2)   # (1: the one edge taken ended the game, no child)
            cells.append((i, j) if visited else ((i + 1) % t["m"], j) if t["m"] > 1 else (i, (j + 1) % t["n"]))
        rows = np.array([q for q, t in enumerate(trees) if visited or t["m"] * t["n"] > 1])
        i, j, obs, res = play(gpu_ctx, trees, bb, dd, cells)
        src = rows[(res[rows] & 15) == 0]
        kept = forest.advance(i[src], j[src], obs[src], src=src)
        counts = forest.node_counts(len(src))
        b2, d2, r2, s2 = np.ascontiguousarray(bb[src]), np.ascontiguousarray(dd[src]), np.ascontiguousarray(res[src]), seeds[src] + np.uint64(77)
        after = forest_search(gpu_ctx, b2, d2, r2, s2, 8, forest=forest, keep=True, solve_nash=True, **kw)
        again = fresh(gpu_ctx, b2, d2, r2, s2, 8, **kw)
        flags = forest.mismatch(len(src))
        if not visited:
            assert len(src) > n // 2 and not kept.any() and (counts == 1).all()
            for a, w in zip(after, again):                                      # an empty tree: the search is a new one, priors included
                same_tree_output(a, w)
                assert np.asarray(a["p1_prior"]).sum() > 0.99 and a["nodes"] == w["nodes"]
            assert not flags.any()
        else:
            # the child the one iteration created was evaluated and initialised by it: a kept, initialised root of one node -- unless the update's
            # observation differs from the iteration's (another damage roll): then there is no such edge
            assert kept.any() and (counts == 1).all()
            for q, (a, w) in enumerate(zip(after, again)):
                if kept[q] and not flags[q]:                                    # no root inference: zero priors, as in the reference
                    assert not np.asarray(a["p1_prior"]).any() and not np.asarray(a["p2_prior"]).any() and a["initial_value"] == 0.0
                    assert int(np.asarray(a["visit_matrix"]).sum()) == 8 and a["iterations"] == 8
                else:
                    same_tree_output(a, w)
        assert forest.keep_stats()[3] == 0
        forest.close()
    net.close()


def test_a_root_with_other_choice_counts_starts_afresh_and_is_flagged(gpu_ctx):
    from oak_amd.search import Forest, forest_search
    n, iterations = 24, 16
    b, d, r, seeds, _ = roots(n)
    bb, dd = b.copy(), d.copy()
    kw = dict(c=1.0, evaluator="poke-engine")
    forest = Forest(gpu_ctx, n, iterations, keep_arena=0)
    trees = forest_search(gpu_ctx, bb, dd, r, seeds, iterations, forest=forest, keep=True, solve_nash=True, **kw)
    i, j, obs, res = play(gpu_ctx, trees, bb, dd)
    kept = forest.advance(i, j, obs)                                            # every row, finished ones too: their trees are empty
    assert not kept[(res & 15) != 0].any() and kept.any()
    # the kept roots' counts, from the trees themselves; then every tree is handed ANOTHER row's position
    k1 = np.array([forest.nodes(q, 0, 1)[0][0][0] for q in range(n)])
    k2 = np.array([forest.nodes(q, 0, 1)[0][1][0] for q in range(n)])
    give = np.roll(np.arange(n), 1)                                             # tree q searches the ORIGINAL position of row give[q]
    b2, d2, r2, s2 = np.ascontiguousarray(b[give]), np.ascontiguousarray(d[give]), np.ascontiguousarray(r[give]), seeds + np.uint64(5)
    after = forest_search(gpu_ctx, b2, d2, r2, s2, iterations, forest=forest, keep=True, solve_nash=True, **kw)
    again = fresh(gpu_ctx, b2, d2, r2, s2, iterations, **kw)
    flags = forest.mismatch(n)
    want = np.array([k1[q] != 0 and (k1[q], k2[q]) != (again[q]["m"], again[q]["n"]) for q in range(n)])
    assert (flags == want).all() and want.any(), (flags, want)
    for q in range(n):
        if flags[q] or k1[q] == 0:
            same_tree_output(after[q], again[q])
    forest.close()


# ---- 3. between rows -------------------------------------------------------------------------------------------------------------------
def test_an_advance_moves_trees_between_rows(gpu_ctx):
    from oak_amd.search import Forest, forest_search
    n, iterations = 40, 16
    b, d, r, seeds, _ = roots(n)
    kw = dict(c=1.0, evaluator="poke-engine")
    outs = {}
    for name in ("identity", "reversed", "every third"):
        bb, dd = b.copy(), d.copy()
        forest = Forest(gpu_ctx, n, iterations, keep_arena=0)
        trees = forest_search(gpu_ctx, bb, dd, r, seeds, iterations, forest=forest, keep=True, solve_nash=True, **kw)
        i, j, obs, res = play(gpu_ctx, trees, bb, dd)
        alive = np.flatnonzero((res & 15) == 0)
        src = {"identity": alive, "reversed": alive[::-1], "every third": alive[::3]}[name]
        kept = forest.advance(i[src], j[src], obs[src], src=src)
        counts = forest.node_counts(len(src))
        nxt = forest_search(gpu_ctx, np.ascontiguousarray(bb[src]), np.ascontiguousarray(dd[src]), np.ascontiguousarray(res[src]), seeds[src] + np.uint64(9),
                            iterations, forest=forest, keep=True, solve_nash=True, **kw)
        roots_after = [forest.nodes(t, 0, 1) for t in range(len(src))]
        outs[name] = {int(g): (kept[t], counts[t], nxt[t], roots_after[t]) for t, g in enumerate(src)}
        assert forest.keep_stats()[3] == 0
        forest.close()
    assert len(outs["identity"]) > 20 and sum(int(v[0]) for v in outs["identity"].values()) > 10
    for name in ("reversed", "every third"):
        for g, (kept, count, tree, root) in outs[name].items():
            k0, c0, t0, r0 = outs["identity"][g]
            assert kept == k0 and count == c0, (name, g)
            same_tree_output(tree, t0)
            assert all(x.tobytes() == y.tobytes() for p, q in zip(root[0], r0[0]) for x, y in zip(p[1:], q[1:])), (name, g)


# ---- 4. capacity -----------------------------------------------------------------------------------------------------------------------
def test_a_subtree_that_leaves_no_room_is_dropped_and_counted(gpu_ctx):
    from oak_amd.search import Forest, forest_search
    n, iterations = 40, 16
    b, d, r, seeds, _ = roots(n)
    kw = dict(c=1.0, evaluator="poke-engine")
    got = {}
    for arena in (0, iterations + 1):
        bb, dd = b.copy(), d.copy()
        forest = Forest(gpu_ctx, n, iterations, keep_arena=arena)
        assert forest.keep_stats()[0] == (4 * iterations + 1 if arena == 0 else arena)
        trees = forest_search(gpu_ctx, bb, dd, r, seeds, iterations, forest=forest, keep=True, solve_nash=True, **kw)
        i, j, obs, res = play(gpu_ctx, trees, bb, dd)
        src = np.flatnonzero((res & 15) == 0)
        kept = forest.advance(i[src], j[src], obs[src], src=src)
        counts = forest.node_counts(len(src))
        b2, d2, r2, s2 = np.ascontiguousarray(bb[src]), np.ascontiguousarray(dd[src]), np.ascontiguousarray(res[src]), seeds[src] + np.uint64(3)
        nxt = forest_search(gpu_ctx, b2, d2, r2, s2, iterations, forest=forest, keep=True, solve_nash=True, **kw)
        got[arena] = (kept, counts, nxt, forest.keep_stats()[3], (b2, d2, r2, s2))
        forest.close()
    kept0, counts0, nxt0, dropped0, _ = got[0]
    kept1, counts1, nxt1, dropped1, (b2, d2, r2, s2) = got[iterations + 1]
    big = (kept0 == 1) & (counts0 >= 2)
    assert dropped0 == 0 and dropped1 == int(big.sum()) > 0
    assert not kept1[big].any() and (kept1[~big] == kept0[~big]).all() and (counts1[big] == 1).all()
    again = fresh(gpu_ctx, b2, d2, r2, s2, iterations, **kw)
    for q in range(len(kept1)):
        same_tree_output(nxt1[q], again[q] if big[q] or not kept0[q] else nxt0[q])


# ---- 5. self-play, UCB: the host loop with keep_node -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["e", "e0.5-n0.5"])
@pytest.mark.parametrize("evaluator, iterations", [("poke-engine", 16), ("mc", 8), ("tiny", 8)])
def test_ucb_games_with_keep_node_are_the_host_loops(gpu_ctx, tmp_path, evaluator, iterations, mode):
    n = 12
    teams, battle_seeds, seeds = games(n, salt=20)
    ev = evaluator_of(gpu_ctx, tmp_path, evaluator)
    stats = {}
    out = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=2.0, evaluator=ev, policy_mode=mode, solve_nash=True, stats=stats, keep_node=True)
    recs, nodes_kept = records(out), out[5]
    assert (out[4] == OK).all() and stats["dropped"] == 0, stats
    assert len(set(int(x) for x in out[2])) > 3                                  # games of differing length: retirement moves trees across rows
    for g in range(n):
        host = {}
        want = selfplay_game(gpu_ctx, teams[g], int(battle_seeds[g]), iterations=iterations, batch=1, c=2.0, evaluator=ev, policy_mode=mode, seed=int(seeds[g]),
                             keep_node=True, stats=host)
        assert recs[g] == want[0], (g, len(recs[g]), len(want[0]))
        assert (int(out[2][g]), int(out[3][g])) == want[1:] and int(nodes_kept[g]) == host["nodes_kept"], (g, nodes_kept[g], host)
    print(evaluator, mode, "frames", out[2], "nodes_kept", nodes_kept, stats)
    assert (nodes_kept > 0).any() and (nodes_kept < out[2]).any()
    assert stats["nodes_kept"] == int(nodes_kept.sum()) and stats["host_reads"] == stats["turns"] + 1
    if not isinstance(ev, str):
        ev.close()


# ---- 6. self-play, PUCB ----------------------------------------------------------------------------------------------------------------
def drive(ctx, net, teams, battle_seeds, seeds, iterations, mode, c):
    """The game loop restated over the standalone calls: search_kept, oakgpu_selfplay_pick_host, update, advance.  Returns the per-game
    update lists and nodes_kept."""
    from oak_amd.search import Forest, forest_search
    n = len(seeds)
    b, d, r = ctx.battle(teams.reshape(n, 2, 6, 5), battle_seeds)
    forest = Forest(ctx, n, iterations, contextual=True, keep_arena=0)
    state = [R.game_stream(int(s)) for s in seeds]
    updates, nodes_kept = [[] for _ in range(n)], np.zeros(n, np.int64)
    live = np.arange(n)
    while len(live):
        tree_seeds = []
        for g in live:
            state[g], s = R.splitmix64(state[g])
            tree_seeds.append(s)
        trees = forest_search(ctx, b, d, r, np.array(tree_seeds, np.uint64), iterations, c=c, bandit="pucb", evaluator=net, solve_nash=True, forest=forest, keep=True)
        flags = forest.mismatch(len(live))
        cells = []
        for q, g in enumerate(live):
            raw = trees[q]["raw"]
            p = selfplay_pick_host(raw.m, raw.n, np.array(raw.visit_matrix, np.uint64), np.array(raw.value_matrix), iterations, state[g], p1_nash=list(raw.p1_nash),
                                   p2_nash=list(raw.p2_nash), nash_value=raw.nash_value, p1_prior=list(raw.p1_prior), p2_prior=list(raw.p2_prior),
                                   p1_choices=list(raw.p1_choices), p2_choices=list(raw.p2_choices), policy_mode=mode)
            state[g] = p["rng"]
            updates[g].append(p["update"])
            cells.append((p["i"], p["j"]))
            if flags[q] and nodes_kept[g]:
                nodes_kept[g] -= 1
        i, j, obs, res = play(ctx, trees, b, d, cells)
        src = np.flatnonzero((res & 15) == 0)
        kept = forest.advance(i[src], j[src], obs[src], src=src)
        nodes_kept[live[src]] += kept
        live, b, d, r = live[src], np.ascontiguousarray(b[src]), np.ascontiguousarray(d[src]), np.ascontiguousarray(res[src])
    assert forest.keep_stats()[3] == 0
    forest.close()
    return updates, nodes_kept


def test_pucb_games_with_keep_node(gpu_ctx, tmp_path):
    iterations, mode, c = 8, "p0.5-e0.5", 1.5
    teams, battle_seeds, seeds = games(70, salt=21)
    net = network(gpu_ctx, tmp_path, "tiny")
    kw = dict(c=c, bandit="pucb", evaluator=net, policy_mode=mode, solve_nash=True, keep_node=True)
    stats = {}
    big = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, stats=stats, **kw)
    assert (big[4] == OK).all() and stats["dropped"] == 0
    rep = replay_check(gpu_ctx, big[0])
    assert len(rep["reports"]) == 70 and (rep["reports"]["status"] == 0).all() and rep["stopped_at"] == len(big[0])
    recs = records(big)
    seven = forest_selfplay(gpu_ctx, teams[:7], battle_seeds[:7], seeds[:7], iterations, **kw)
    assert records(seven) == recs[:7] and (seven[5] == big[5][:7]).all() and (seven[2] == big[2][:7]).all()
    for g in (3, 69):
        one = forest_selfplay(gpu_ctx, teams[g:g + 1], battle_seeds[g:g + 1], seeds[g:g + 1], iterations, **kw)
        assert one[0] == recs[g] and int(one[5][0]) == int(big[5][g]), g
    updates, nodes_kept = drive(gpu_ctx, net, teams[:7], battle_seeds[:7], seeds[:7], iterations, mode, c)
    for g in range(7):
        assert R.split_updates(recs[g]) == updates[g], g
    assert (nodes_kept == seven[5]).all() and (seven[5] > 0).any(), (nodes_kept, seven[5])
    print("pucb keep_node: frames", big[2][:7], "nodes_kept", big[5][:7], stats)
    net.close()


# ---- 7. the calls around it ------------------------------------------------------------------------------------------------------------
def test_keep_node_off_on_a_kept_forest_is_the_plain_forests_stream(gpu_ctx):
    from oak_amd.search import Forest
    n, iterations = 9, 8
    teams, battle_seeds, seeds = games(n, salt=22)
    kw = dict(c=2.0, evaluator="poke-engine", policy_mode="e", solve_nash=True)
    want = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, **kw)
    kept = Forest(gpu_ctx, n, iterations, keep_arena=0)
    forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, forest=kept, keep_node=True, **kw)   # a kept game first: its trees are left behind
    got = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, forest=kept, **kw)
    assert got[0] == want[0] and all((a == b).all() for a, b in zip(got[1:], want[1:]))
    again = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, forest=kept, keep_node=True, **kw)
    first = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, keep_node=True, **kw)
    assert again[0] == first[0] and (again[5] == first[5]).all()               # and a kept game does not depend on what the forest held
    kept.close()


def test_a_plain_forest_refuses_the_kept_calls_by_name(gpu_ctx):
    from oak_amd.search import Forest, forest_search
    b, d, r, seeds, _ = roots(4)
    plain = Forest(gpu_ctx, 4, 8)
    with pytest.raises(OakGpuError, match="oakgpu_forest_advance: the forest was created without keep"):
        plain.advance(np.zeros(4, np.uint8), np.zeros(4, np.uint8), np.zeros((4, 16), np.uint8))
    with pytest.raises(OakGpuError, match="oakgpu_forest_search_kept: the forest was created without keep"):
        forest_search(gpu_ctx, b, d, r, seeds, 8, evaluator="poke-engine", forest=plain, keep=True)
    with pytest.raises(OakGpuError, match="created without keep"):
        plain.keep_stats()
    teams, battle_seeds, game_seeds = games(4)
    with pytest.raises(OakGpuError, match="keep_node is not supported on this forest.*oakgpu_forest_create_kept"):
        forest_selfplay(gpu_ctx, teams, battle_seeds, game_seeds, 8, evaluator="poke-engine", forest=plain, keep_node=True)
    forest_search(gpu_ctx, b, d, r, seeds, 8, evaluator="poke-engine", forest=plain)   # and it still serves the plain call
    plain.close()


# ---- 8. faces ----------------------------------------------------------------------------------------------------------------------------
def test_pyoak_face_with_keep_node_equals_the_c_call(gpu_ctx):
    from oak_amd import pyoak
    n, iterations = 7, 8
    teams, battle_seeds, seeds = games(n, salt=23)
    want = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=1.0, evaluator="poke-engine", policy_mode="e0.9-x0.1", keep_node=True)
    agent = pyoak.Agent()
    agent.budget, agent.bandit, agent.eval = str(iterations), "ucb-1.0", "fp"
    got = pyoak.selfplay_forest(teams, battle_seeds, seeds, agent, policy_mode="e0.9-x0.1", keep_node=True)
    assert len(got) == 6 and got[0] == want[0] and all((np.asarray(a) == b).all() for a, b in zip(got[1:], want[1:])) and want[5].any()
    assert len(pyoak.selfplay_forest(teams, battle_seeds, seeds, agent, policy_mode="e0.9-x0.1")) == 5
    with pytest.raises(RuntimeError, match="keep_arena must be at least max_iterations \\+ 1"):
        pyoak.selfplay_forest(teams, battle_seeds, seeds, agent, keep_node=True, keep_arena=iterations)


def test_torch_face_in_a_child_process():
    """The kept calls with torch tensors on the device, through tests/forest_keep_torch_check.py in a child process -- torch must initialise
    the GPU before the library does."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "forest_keep_torch_check.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "forest keep torch ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
