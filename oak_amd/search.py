"""Nash-at-root search fed by GPU batches (BASELINE config 5) -- host-side consumer of the hot path.

Mirrors two pieces of the reference's search surface:
  * `solve_matrix(payoffs, discretize_factor) -> (p1, p2, value)`  (pyoak: cpp/src/pyoak.cc:394-426; used by
    MCTS::Search::process_output, cpp/include/search/mcts.h:620-659, through the absent lrsnash/GMP library):
    exact Nash equilibrium of a <= 9 x 9 one-sum matrix game with integer payoffs -- a thin call into the C ABI
    (oakgpu_solve_matrix: integer-pivoting simplex, Bland's rule, no floating point in the solve).
  * `solve_matrices(ctx, matrices, discretize_factor)`: a batch of those on the GPU, one workgroup per matrix, the same bits
    (oakgpu_solve_matrices, oak_amd/csrc/nashdev.hip).
  * `root_matrix_search(...)`: for every joint action (i, j) of the root and R replicas, re-seed + resample hidden
    counters (mcts.h:254-259), apply the joint action with ONE batched update on the GPU, evaluate the R x m x n
    children with GPU rollouts (or the GPU network), average into the value matrix and solve it.  Output fields
    follow MCTS::Output (mcts.h:68-90).
  * `tree_search(...)`: the full tree search -- MCTS::Search::run (mcts.h:154-247) with a Node heap and joint
    UCB / PUCB bandits -- as `oakgpu_search` runs it: batches of descents walking a host-side tree, every battle
    state resident on the GPU (oak_amd/csrc/search_host.hip), process_output's Nash solve included.
All battle arithmetic runs through the C ABI (oak_amd.engine); this module only orchestrates and solves.
"""
import ctypes as C

import numpy as np

from . import _lib


def solve_matrix(payoffs, discretize_factor=256):
    """pyoak `solve_matrix` (pyoak.cc:394-426) over oakgpu_solve_matrix (exact integer-pivoting simplex in C++,
    oak_amd/csrc/nash.hpp).  payoffs: m x n integers = value * discretize_factor (the row player's one-sum payoff).
    Returns (p1 float[m], p2 float[n], value float)."""
    P = np.asarray(payoffs)
    if P.ndim != 2 or P.shape[0] < 1 or P.shape[1] < 1 or P.shape[0] > 9 or P.shape[1] > 9:
        raise RuntimeError("solve_matrix: payoff matrix must be between 1x1 and 9x9")
    m, n = P.shape
    M = np.ascontiguousarray(P, dtype=np.int32)
    p1, p2, v = np.zeros(m), np.zeros(n), C.c_double(0)
    _lib.check(_lib.load().oakgpu_solve_matrix(M.ctypes.data_as(C.c_void_p), m, n, int(discretize_factor), p1.ctypes.data_as(C.c_void_p),
                                               p2.ctypes.data_as(C.c_void_p), C.cast(C.byref(v), C.c_void_p)))
    return p1, p2, v.value


def solve_matrices(ctx, matrices, discretize_factor=256):
    """A batch of solve_matrix calls on the GPU (oakgpu_solve_matrices: one workgroup per matrix, oak_amd/csrc/nashdev.hip): entry k is
    solve_matrix(matrices[k], discretize_factor) bit for bit, and what that call refuses fails the whole call.  matrices: a sequence of
    m x n integer arrays (shapes may differ).  Returns a list of (p1 float[m], p2 float[n], value float)."""
    mats = [np.asarray(P) for P in matrices]
    count = len(mats)
    pay, ms, ns = np.zeros((max(count, 1), 81), np.int32), np.zeros(max(count, 1), np.int32), np.zeros(max(count, 1), np.int32)
    for k, P in enumerate(mats):
        if P.ndim != 2 or P.shape[0] < 1 or P.shape[1] < 1 or P.shape[0] > 9 or P.shape[1] > 9:
            raise RuntimeError("solve_matrices: matrix %d: payoff matrix must be between 1x1 and 9x9" % k)
        ms[k], ns[k] = P.shape
        pay[k, :P.size] = np.ascontiguousarray(P, dtype=np.int32).reshape(-1)
    p1, p2, v = np.zeros((max(count, 1), 9)), np.zeros((max(count, 1), 9)), np.zeros(max(count, 1))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(ctx.lib.oakgpu_solve_matrices(ctx.handle, vp(pay), vp(ms), vp(ns), count, int(discretize_factor), vp(p1), vp(p2), vp(v)))
    return [(p1[k, :ms[k]].copy(), p2[k, :ns[k]].copy(), float(v[k])) for k in range(count)]


def root_matrix_search(ctx, battle, durations, result, replicas=256, seed=0x5EED, evaluator="mc", max_steps=1000):
    """One-ply Nash-at-root search of a position (battle uint8[384], durations uint8[8], result byte).

    evaluator: "mc" (random rollouts on the GPU, MCTS::MonteCarlo) or an oak_amd.engine.Network
    (value_inference on the GPU).  Returns a dict shaped like MCTS::Output (mcts.h:68-90)."""
    battle = np.ascontiguousarray(battle, dtype=np.uint8).reshape(1, 384)
    durations = np.ascontiguousarray(durations, dtype=np.uint8).reshape(1, 8)
    res = np.array([result], dtype=np.uint8)
    c1, n1 = ctx.choices(battle, res, 0)
    c2, n2 = ctx.choices(battle, res, 1)
    m, n = int(n1[0]), int(n2[0])
    lanes = m * n * replicas
    B = np.repeat(battle, lanes, axis=0)
    D = np.repeat(durations, lanes, axis=0)
    R = np.repeat(res, lanes)
    # one fast_prng stream per lane (util/random.h:67-133); seeded counter-style, state never all-zero
    rng = np.random.default_rng(seed)
    prng = rng.integers(0, 256, (lanes, 8), dtype=np.uint8)
    prng[:, 0] |= 1
    # root-iteration prep on the device (mcts.h:254-259): max_steps = 0 -> only re-seed + hidden-variable resampling
    prepped = ctx.rollout(B, D, R, prng, max_steps=0, prep=True, return_state=True)
    B, D, prng = prepped["battles"], prepped["durations"], prepped["prng"]
    ii, jj = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    a1 = np.repeat(c1[0, ii.ravel()], replicas)
    a2 = np.repeat(c2[0, jj.ravel()], replicas)
    child_res, _ = ctx.update(B, a1, a2, D, want_actions=False)          # in place on B, D
    t = child_res & 15
    values = np.where(t == 1, 1.0, np.where(t == 2, 0.0, 0.5)).astype(np.float32)
    live = t == 0
    if live.any():
        if evaluator == "mc":
            out = ctx.rollout(B[live], D[live], child_res[live], prng[live], max_steps=max_steps)
            values[live] = out["values"]
        else:
            values[live] = evaluator.value_inference(B[live], D[live])
    cum = values.reshape(m, n, replicas).sum(axis=2).astype(np.float64)
    visits = np.full((m, n), replicas, dtype=np.int64)
    mean = cum / visits
    p1, p2, nash_value = solve_matrix(np.floor(mean * 256).astype(np.int64), 256)   # mcts.h:631-633: value / n * 256 as int
    return {
        "m": m, "n": n, "p1_choices": c1[0, :m].copy(), "p2_choices": c2[0, :n].copy(),
        "visit_matrix": visits, "value_matrix": cum,                       # cumulative, like the reference (mcts.h:80-81)
        "iterations": lanes, "empirical_value": float(values.mean()), "nash_value": nash_value,
        "p1_nash": p1, "p2_nash": p2,
        "p1_empirical": np.full(m, 1.0 / m), "p2_empirical": np.full(n, 1.0 / n),
    }


def process_output(out):
    """MCTS::Search::process_output (mcts.h:620-659) on a dict holding m, n, visit_matrix, value_matrix, iterations:
    adds nash_value / p1_nash / p2_nash (empirical matrix x 256 as integers, exact solve) and the empirical fields."""
    m, n = out["m"], out["n"]
    visits = np.asarray(out["visit_matrix"])[:m, :n].astype(np.int64)
    values = np.asarray(out["value_matrix"])[:m, :n].astype(np.float64)
    nn = np.where(visits == 0, 1, visits)
    p1, p2, nash = solve_matrix((values / nn * 256).astype(np.int64), 256)   # C++ double -> int truncation
    it = max(int(out["iterations"]), 1)
    out.update(nash_value=nash, p1_nash=p1, p2_nash=p2, empirical_value=float(values.sum() / it),
               p1_empirical=visits.sum(axis=1) / it, p2_empirical=visits.sum(axis=0) / it)
    return out


class Heap:
    """RuntimeSearch::Heap (util/search.h:17-32, search.cc:17-58) over oakgpu_heap: the tree of a search, kept between
    searches.  empty() is True until a search used it; update(i, j, obs) promotes the child reached by the PLAYED joint
    action (indices into the root's choice lists) and the 16-byte observation to the root, dropping the rest."""

    def __init__(self):
        self.lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self.lib.oakgpu_heap_create(C.byref(h)))
        self.handle = h

    def empty(self):
        return bool(self.lib.oakgpu_heap_empty(self.handle))

    def nodes(self):
        return int(self.lib.oakgpu_heap_nodes(self.handle))

    def clear(self):
        self.lib.oakgpu_heap_clear(self.handle)

    def shard_violations(self):
        """Edges whose child sits in another table's arena (oakgpu_heap_check_shards): 0 in a consistent tree."""
        return int(self.lib.oakgpu_heap_check_shards(self.handle))

    def update(self, i, j, obs):
        o = np.ascontiguousarray(obs, dtype=np.uint8).reshape(16)
        return bool(self.lib.oakgpu_heap_update(self.handle, int(i), int(j), o.ctypes.data_as(C.c_void_p)))

    def root_stats(self, player):
        """(scores[k], priors[k], visits[k]) of the root's bandit of `player` (0 / 1); k = 0: the root is not initialised."""
        sc, pr, vi, k = np.zeros(9, np.float32), np.zeros(9, np.float32), np.zeros(9, np.uint32), C.c_uint8(0)
        _lib.check(self.lib.oakgpu_heap_root_stats(self.handle, int(player), sc.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p),
                                                   vi.ctypes.data_as(C.c_void_p), C.cast(C.byref(k), C.c_void_p)))
        return sc[:k.value].copy(), pr[:k.value].copy(), vi[:k.value].copy()

    def child_stats(self, i, j, obs, player):
        """root_stats of the child that update(i, j, obs) would promote (empty arrays: no such initialised child)."""
        o = np.ascontiguousarray(obs, dtype=np.uint8).reshape(16)
        sc, pr, vi, k = np.zeros(9, np.float32), np.zeros(9, np.float32), np.zeros(9, np.uint32), C.c_uint8(0)
        _lib.check(self.lib.oakgpu_heap_child_stats(self.handle, int(i), int(j), o.ctypes.data_as(C.c_void_p), int(player),
                                                    sc.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p), vi.ctypes.data_as(C.c_void_p),
                                                    C.cast(C.byref(k), C.c_void_p)))
        return sc[:k.value].copy(), pr[:k.value].copy(), vi[:k.value].copy()

    def close(self):
        if self.handle:
            self.lib.oakgpu_heap_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _output_dict(res):
    m, n = int(res.m), int(res.n)
    return {"m": m, "n": n, "p1_choices": np.array(res.p1_choices[:m], dtype=np.uint8),
            "p2_choices": np.array(res.p2_choices[:n], dtype=np.uint8),
            "visit_matrix": np.array(res.visit_matrix, dtype=np.int64).reshape(9, 9)[:m, :n].copy(),
            "value_matrix": np.array(res.value_matrix, dtype=np.float64).reshape(9, 9)[:m, :n].copy(),
            "iterations": int(res.iterations), "initial_value": float(res.initial_value), "nodes": int(res.nodes),
            "mean_depth": res.total_depth / max(int(res.iterations), 1), "duration_ms": res.duration_us / 1e3,
            # process_output ran in C++ (oakgpu_search_output: exact Nash of the empirical root matrix)
            "nash_value": float(res.nash_value), "p1_nash": np.array(res.p1_nash[:m]), "p2_nash": np.array(res.p2_nash[:n]),
            "empirical_value": float(res.empirical_value), "p1_empirical": np.array(res.p1_empirical[:m]),
            "p2_empirical": np.array(res.p2_empirical[:n]),
            "p1_logit": np.array(res.p1_logit[:m]), "p2_logit": np.array(res.p2_logit[:n]),
            "p1_prior": np.array(res.p1_prior[:m]), "p2_prior": np.array(res.p2_prior[:n]),
            "raw": res}          # the oakgpu_search_output itself: pass the dict back as `previous` to resume (mcts.h:153-155)


def tree_search_many(ctxs, battles, durations, results, seeds, iterations=1 << 16, batch=4096, c=2.0, bandit="ucb", evaluator="mc",
                     root_rolls=3, other_rolls=1, max_depth=100, alpha=0.05, heaps=None, threads_per_search=0):
    """n independent tree searches at once on one GPU (include/oakgpu.h: oakgpu_search_many): search i runs on ctxs[i] (a Context of its
    own each) from battles[i] with seeds[i]; heaps: None or one Heap per search.  Returns the list of output dicts -- each identical to
    tree_search(ctxs[i], battles[i], ..., seed=seeds[i]) run alone."""
    n = len(ctxs)
    battles = np.ascontiguousarray(battles, dtype=np.uint8).reshape(n, 384)
    durations = np.ascontiguousarray(durations, dtype=np.uint8).reshape(n, 8)
    results = np.ascontiguousarray(results, dtype=np.uint8).reshape(n)
    use_net = not isinstance(evaluator, str)
    prms = (_lib.SearchParams * n)()
    for i in range(n):
        prms[i] = _lib.SearchParams(iterations=int(iterations), batch=int(batch), ucb_c=float(c), bandit={"ucb": 0, "pucb": 1, "ucb1": 2, "exp3": 3, "pexp3": 4}[bandit],
                                    eval=1 if use_net else {"mc": 0, "poke-engine": 2}[evaluator], max_depth=int(max_depth), root_rolls=int(root_rolls),
                                    other_rolls=int(other_rolls), seed=int(seeds[i]), matrix_ucb=0, mucb_delay=0, mucb_minimum=0, mucb_c=0.0,
                                    exp3_alpha=float(alpha), duration_us=0)
    outs = (_lib.SearchOutput * n)()
    cp = (C.c_void_p * n)(*[c_.handle for c_ in ctxs])
    hp = (C.c_void_p * n)(*[h.handle for h in heaps]) if heaps is not None else None
    _lib.check(ctxs[0].lib.oakgpu_search_many(cp, evaluator.handle if use_net else None, hp, battles.ctypes.data_as(C.c_void_p),
                                              durations.ctypes.data_as(C.c_void_p), results.ctypes.data_as(C.c_void_p), prms, n, int(threads_per_search), outs))
    res = []
    for i in range(n):   # (_output_dict keeps a reference to its raw struct: give each its own copy)
        o = _lib.SearchOutput()
        C.memmove(C.byref(o), C.byref(outs[i]), C.sizeof(_lib.SearchOutput))
        res.append(_output_dict(o))
    return res


def tree_search(ctx, battle, durations, result, iterations=1 << 16, batch=4096, c=2.0, bandit="ucb", evaluator="mc",
                root_rolls=3, other_rolls=1, max_depth=100, seed=0x5EED, matrix_ucb=None, alpha=0.05, heap=None, previous=None,
                duration_us=0):
    """Tree search with batched leaves on the GPU (include/oakgpu.h: oakgpu_search_heap).  bandit: "ucb" | "pucb" | "ucb1" | "exp3" | "pexp3" (c = gamma for the Exp3 family, alpha its uniform mixing);
    evaluator: "mc", "poke-engine" (PokeEngine::Eval) or an oak_amd.engine.Network.  Defaults follow the reference's default_search{3, 1} damage-roll
    clamping (mcts.h:131).  matrix_ucb: None or (delay, minimum, c) -- MatrixUCBParams with interval = batch (the
    reference's "delay-interval-minimum-c" agent string, search.cc:216-231).  heap: None (fresh tree) or a Heap kept between
    searches; previous: None or the dict a previous tree_search of the SAME position returned -- matrices, iterations and
    duration accumulate like MCTS::Search::run's by-value Output (mcts.h:153-155, 231-247).  Returns a dict shaped like
    MCTS::Output (mcts.h:68-90)."""
    battle = np.ascontiguousarray(battle, dtype=np.uint8).reshape(384)
    durations = np.ascontiguousarray(durations, dtype=np.uint8).reshape(8)
    use_net = not isinstance(evaluator, str)
    prm = _lib.SearchParams(iterations=int(iterations), batch=int(batch), ucb_c=float(c), bandit={"ucb": 0, "pucb": 1, "ucb1": 2, "exp3": 3, "pexp3": 4}[bandit],
                            eval=1 if use_net else {"mc": 0, "poke-engine": 2}[evaluator], max_depth=int(max_depth), root_rolls=int(root_rolls),
                            other_rolls=int(other_rolls), seed=int(seed), matrix_ucb=1 if matrix_ucb else 0,
                            mucb_delay=int(matrix_ucb[0]) if matrix_ucb else 0, mucb_minimum=int(matrix_ucb[1]) if matrix_ucb else 0,
                            mucb_c=float(matrix_ucb[2]) if matrix_ucb else 0.0, exp3_alpha=float(alpha), duration_us=int(duration_us))
    res = _lib.SearchOutput()
    prev = C.byref(previous["raw"]) if previous is not None else None
    _lib.check(ctx.lib.oakgpu_search_heap(ctx.handle, evaluator.handle if use_net else None, heap.handle if heap is not None else None,
                                          battle.ctypes.data_as(C.c_void_p), durations.ctypes.data_as(C.c_void_p), int(result), C.byref(prm),
                                          prev, C.byref(res)))
    return _output_dict(res)


def search_stream(ctx):
    """The continuing fast_prng state of the last tree_search on `ctx` (lane 0 of its first batch slot; with batch = 1 its one stream)."""
    s = C.c_uint64(0)
    _lib.check(ctx.lib.oakgpu_search_stream(ctx.handle, C.byref(s)))
    return int(s.value)


TRACE_HEAD_BYTES = C.sizeof(_lib.ForestTraceHead)


def trace_dtype(trace_levels):
    """numpy dtype of one trace record of the forest search (include/oakgpu.h: oakgpu_forest_trace_head + trace_levels levels)."""
    level = np.dtype([("node", "<u4"), ("i", "u1"), ("j", "u1"), ("pad", "u1", (2,))])
    return np.dtype([("levels", "<u4"), ("leaf", "<u4"), ("initialised", "u1"), ("result_type", "u1"), ("pad", "u1", (2,)), ("value", "<f4"),
                     ("logits", "<f4", (2, 9)), ("path", level, (int(trace_levels),))])


class Forest:
    """oakgpu_forest: the device arenas of `max_trees` trees of up to `max_iterations` iterations each (include/oakgpu.h); contextual =
    room for the policy logits PUCB needs.  Kept between forest_search calls to save the allocation.
    keep_arena: None = a plain forest; a node count per tree (0 = 4 * max_iterations + 1) = a kept forest (oakgpu_forest_create_kept),
    whose trees go on from call to call: forest_search(..., keep=True) and advance()."""

    def __init__(self, ctx, max_trees, max_iterations, contextual=False, keep_arena=None):
        self.ctx, self.max_trees, self.max_iterations, self.contextual = ctx, int(max_trees), int(max_iterations), bool(contextual)
        self.kept = keep_arena is not None
        h = C.c_void_p()
        if self.kept:
            _lib.check(ctx.lib.oakgpu_forest_create_kept(ctx.handle, self.max_trees, self.max_iterations, int(self.contextual), int(keep_arena), C.byref(h)))
        else:
            _lib.check(ctx.lib.oakgpu_forest_create(ctx.handle, self.max_trees, self.max_iterations, int(self.contextual), C.byref(h)))
        self.handle = h

    def advance(self, i, j, obs, src=None):
        """Heap::update of every tree, and its move to another row (oakgpu_forest_advance*): new tree t continues tree src[t] (None: tree t)
        of the last call along the played cell (i[t], j[t]) and the update's 16-byte observation obs[t].  Returns kept [n] uint8: 1 = the
        child is the root now with its whole subtree, 0 = nothing kept (an empty tree).  torch GPU tensors in (uint8 i, j, obs [n, 16];
        int32 src): a tensor out, nothing copied to the host."""
        lib = self.ctx.lib
        if hasattr(i, "data_ptr"):
            import torch
            n, dev = int(i.shape[0]), i.device
            i, j, obs = i.contiguous(), j.contiguous(), obs.contiguous()
            src = None if src is None else src.to(torch.int32).contiguous()
            kept = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
            mine, theirs = torch.cuda.ExternalStream(self.ctx.stream_ptr(), device=dev), torch.cuda.current_stream(dev)
            mine.wait_stream(theirs)
            _lib.check(lib.oakgpu_forest_advance_dev(self.handle, i.data_ptr(), j.data_ptr(), obs.data_ptr(), None if src is None else src.data_ptr(), n,
                                                     kept.data_ptr()))
            theirs.wait_stream(mine)
            self._counts = None
            return kept[:n]
        i = np.ascontiguousarray(i, dtype=np.uint8).reshape(-1)
        n = len(i)
        j = np.ascontiguousarray(j, dtype=np.uint8).reshape(n)
        obs = np.ascontiguousarray(obs, dtype=np.uint8).reshape(n, 16)
        src = None if src is None else np.ascontiguousarray(src, dtype=np.uint32).reshape(n)
        kept = np.zeros(max(n, 1), np.uint8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(lib.oakgpu_forest_advance(self.handle, vp(i), vp(j), vp(obs), None if src is None else vp(src), n, vp(kept)))
        self._counts = None
        return kept[:n]

    def mismatch(self, n):
        """The last kept search's per-tree bytes: 1 = the kept root had other choice counts than the position, the tree started afresh."""
        out = np.zeros(max(int(n), 1), np.uint8)
        _lib.check(self.ctx.lib.oakgpu_forest_mismatch(self.handle, out.ctypes.data_as(C.c_void_p), int(n), 0))
        return out[:int(n)]

    def node_counts(self, n):
        """Node counts of the first n trees the last call (a search or an advance) left."""
        out = np.zeros(max(int(n), 1), np.uint32)
        _lib.check(self.ctx.lib.oakgpu_forest_node_counts(self.handle, out.ctypes.data_as(C.c_void_p), int(n), 0))
        return out[:int(n)]

    def keep_stats(self):
        """(keep_arena, slots per tree, advance launches, trees dropped for want of room) since the forest was made."""
        out = (C.c_uint64 * 4)()
        _lib.check(self.ctx.lib.oakgpu_forest_keep_stats(self.handle, C.byref(out)))
        return tuple(int(x) for x in out)

    def nodes(self, tree, first=0, count=None):
        """Node records of one tree of the last call, in creation order (the root first): a list of ((k, scores, priors, visits) of p1, of p2)."""
        if count is None:
            count = self.node_count(tree) - first
        buf = (_lib.ForestNode * max(count, 1))()
        _lib.check(self.ctx.lib.oakgpu_forest_nodes(self.handle, int(tree), int(first), int(count), buf))
        def side(b):
            return (int(b.k), np.array(b.scores, dtype=np.float32), np.array(b.priors, dtype=np.float32), np.array(b.visits, dtype=np.uint32))
        return [(side(buf[q].p1), side(buf[q].p2)) for q in range(count)]

    def node_count(self, tree):
        if getattr(self, "_counts", None) is None:   # (after an advance: ask for nodes with an explicit count)
            raise ValueError("Forest.nodes: give a count (the node counts are those of the last search)")
        return int(self._counts[int(tree)])

    def last_stats(self):
        """(iterations, tree levels stepped, kernel launches, host reads of the live count) of the last call."""
        out = (C.c_uint64 * 4)()
        _lib.check(self.ctx.lib.oakgpu_forest_last_stats(self.handle, C.byref(out)))
        return tuple(int(x) for x in out)

    def last_rows(self):
        """(tree-iterations launched, tree-iterations run) of the last search: the sum over the iterations of the rows their launches covered,
        and the sum of the trees' budgets; equal when the budgets do not increase in row order, and after every call without budgets."""
        out = (C.c_uint64 * 2)()
        _lib.check(self.ctx.lib.oakgpu_forest_last_rows(self.handle, C.byref(out)))
        return int(out[0]), int(out[1])

    def close(self):
        if self.handle:   # (a forest that outlived its context still frees its arenas: the library then waits for the device)
            self.ctx.lib.oakgpu_forest_destroy(self.ctx.handle, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_FOREST_TENSORS = (("m", "uint8", ()), ("n", "uint8", ()), ("p1_choices", "uint8", (9,)), ("p2_choices", "uint8", (9,)), ("visit_matrix", "int64", (9, 9)),
                   ("value_matrix", "float64", (9, 9)), ("iterations", "int64", ()), ("nodes", "int64", ()), ("total_depth", "int64", ()),
                   ("initial_value", "float64", ()), ("p1_logit", "float64", (9,)), ("p2_logit", "float64", (9,)), ("p1_prior", "float64", (9,)),
                   ("p2_prior", "float64", (9,)), ("stream", "int64", ()))


def forest_search(ctx, battles, durations, results, seeds, iterations, c=2.0, bandit="ucb", evaluator="mc", max_depth=0, root_rolls=3,
                  other_rolls=1, solve_nash=False, trace_levels=0, forest=None, keep=False, budgets=None):
    """n searches at once, one GPU lane per tree, every tree on the device (include/oakgpu.h: oakgpu_forest_search*): tree g is
    tree_search(ctx, battles[g], durations[g], results[g], iterations, batch=1, seed=seeds[g], ...) iteration for iteration.  bandit "ucb" |
    "pucb"; evaluator "mc", "poke-engine" or a Network; forest: None (one made for this call) or a Forest to reuse.
    keep=True (a Forest made with keep_arena): the kept form, oakgpu_forest_search_kept* -- every tree goes on where the forest's last call
    or Forest.advance left it, as tree_search does on a heap; an initialised root is left alone and the outputs' priors are zeros.
    numpy arrays in: a list of n dicts with tree_search's keys (nash fields only with solve_nash; "device" or 2 solves all n
    root matrices in one launch on the GPU, the same bits) plus "stream" (the tree's continuing
    fast_prng state) and, with trace_levels > 0, "trace" (iterations records of trace_dtype(trace_levels)) and -- when the call made its own
    forest -- "tree" (Forest.nodes of the tree: with a forest of the caller's, read them from it).
    torch GPU tensors in (battles [n, 384], durations [n, 8], results [n] uint8; seeds [n] int64 bit patterns): a dict of tensors on that
    device, one row per tree -- m, n, p1_choices, p2_choices, visit_matrix [n, 9, 9], value_matrix, iterations, nodes, total_depth,
    initial_value, p1_logit, p2_logit, p1_prior, p2_prior, stream (int64 bit patterns), and "trace" (uint8 [n, iterations, record bytes])
    with trace_levels > 0; nothing is copied to the host.
    budgets (None, or n x uint32; a torch int32 GPU tensor with tensors in): tree g runs budgets[g] iterations, 1 <= budgets[g] <=
    iterations, and is bit for bit the tree of a call with iterations = budgets[g] (oakgpu_forest_search_budgets*); `iterations` sizes the
    trace, whose records past a tree's budget stay zero.  Rows of non-increasing budgets cost no launch over a finished tree
    (Forest.last_rows())."""
    use_net = not isinstance(evaluator, str)
    prm = _lib.SearchParams(iterations=int(iterations), batch=1, ucb_c=float(c), bandit={"ucb": 0, "pucb": 1, "ucb1": 2, "exp3": 3, "pexp3": 4}[bandit],
                            eval=1 if use_net else {"mc": 0, "poke-engine": 2}[evaluator], max_depth=int(max_depth), root_rolls=int(root_rolls),
                            other_rolls=int(other_rolls), seed=0, matrix_ucb=0, mucb_delay=0, mucb_minimum=0, mucb_c=0.0, exp3_alpha=-1.0, duration_us=0)
    net = evaluator.handle if use_net else None
    on_device = hasattr(battles, "data_ptr")
    n = int(battles.shape[0]) if on_device else len(np.asarray(results).reshape(-1))
    own = forest is None
    if own:
        forest = Forest(ctx, max(n, 1), max(int(iterations), 1), contextual=bandit == "pucb")
    rec = C.sizeof(_lib.ForestTraceHead) + int(trace_levels) * C.sizeof(_lib.ForestTraceLevel)
    try:
        if on_device:
            import torch
            dev = battles.device
            battles, durations, results, seeds = battles.contiguous(), durations.contiguous(), results.contiguous(), seeds.contiguous()
            out = {name: torch.zeros((n,) + tail, dtype=getattr(torch, dt), device=dev) for name, dt, tail in _FOREST_TENSORS}
            trace = torch.zeros((n, int(iterations), rec), dtype=torch.uint8, device=dev) if trace_levels else None
            ptrs = _lib.ForestOutputs(**{name: out[name].data_ptr() for name, _, _ in _FOREST_TENSORS})
            mine, theirs = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev), torch.cuda.current_stream(dev)
            mine.wait_stream(theirs)
            if budgets is not None:
                budgets = budgets.to(torch.int32).contiguous()
                if int(budgets.numel()) != n:
                    raise ValueError("forest_search: one budget per tree")
                _lib.check((ctx.lib.oakgpu_forest_search_budgets_kept_dev if keep else ctx.lib.oakgpu_forest_search_budgets_dev)(
                    forest.handle, net, C.byref(prm), battles.data_ptr(), durations.data_ptr(), results.data_ptr(), seeds.data_ptr(), budgets.data_ptr(), n,
                    C.byref(ptrs), trace.data_ptr() if trace_levels else None, int(trace_levels)))
            else:
                _lib.check((ctx.lib.oakgpu_forest_search_kept_dev if keep else ctx.lib.oakgpu_forest_search_dev)(forest.handle, net, C.byref(prm), battles.data_ptr(), durations.data_ptr(), results.data_ptr(),
                                                        seeds.data_ptr(), n, C.byref(ptrs), trace.data_ptr() if trace_levels else None, int(trace_levels)))
            theirs.wait_stream(mine)
            if trace_levels:
                out["trace"] = trace
            forest._counts = out["nodes"]
            return out
        battles = np.ascontiguousarray(battles, dtype=np.uint8).reshape(n, 384)
        durations = np.ascontiguousarray(durations, dtype=np.uint8).reshape(n, 8)
        results = np.ascontiguousarray(results, dtype=np.uint8).reshape(n)
        seeds = np.ascontiguousarray(np.asarray(seeds).astype(np.uint64)).reshape(n)
        outs = (_lib.SearchOutput * max(n, 1))()
        streams = np.zeros(max(n, 1), np.uint64)
        trace = np.zeros((n, int(iterations)), dtype=trace_dtype(trace_levels)) if trace_levels else None
        if budgets is not None:
            budgets = np.ascontiguousarray(np.asarray(budgets).astype(np.uint32)).reshape(-1)
            if len(budgets) != n:
                raise ValueError("forest_search: one budget per tree")
            _lib.check((ctx.lib.oakgpu_forest_search_budgets_kept if keep else ctx.lib.oakgpu_forest_search_budgets)(
                forest.handle, net, C.byref(prm), battles.ctypes.data_as(C.c_void_p), durations.ctypes.data_as(C.c_void_p), results.ctypes.data_as(C.c_void_p),
                seeds.ctypes.data_as(C.c_void_p), budgets.ctypes.data_as(C.c_void_p), n, outs, _lib.nash_mode(solve_nash), streams.ctypes.data_as(C.c_void_p),
                trace.ctypes.data_as(C.c_void_p) if trace_levels else None, int(trace_levels)))
        else:
            _lib.check((ctx.lib.oakgpu_forest_search_kept if keep else ctx.lib.oakgpu_forest_search)(forest.handle, net, C.byref(prm), battles.ctypes.data_as(C.c_void_p), durations.ctypes.data_as(C.c_void_p),
                                                results.ctypes.data_as(C.c_void_p), seeds.ctypes.data_as(C.c_void_p), n, outs, _lib.nash_mode(solve_nash),
                                                streams.ctypes.data_as(C.c_void_p), trace.ctypes.data_as(C.c_void_p) if trace_levels else None,
                                                int(trace_levels)))
        res = []
        for g in range(n):   # (_output_dict keeps a reference to its raw struct: give each its own copy)
            o = _lib.SearchOutput()
            C.memmove(C.byref(o), C.byref(outs[g]), C.sizeof(_lib.SearchOutput))
            d = _output_dict(o)
            d["stream"] = int(streams[g])
            if trace_levels:
                d["trace"] = trace[g]
            res.append(d)
        forest._counts = [r["nodes"] for r in res]
        if not own:
            return res
        for g, d in enumerate(res):   # the forest goes with the call: its trees are read out now
            d["tree"] = forest.nodes(g) if trace_levels else None
        return res
    finally:
        if own:
            forest.close()


def forest_budgets_check(budgets, iterations):
    """oakgpu_forest_budgets_check alone (host only, no GPU): raises OakGpuError naming the lowest tree whose budget is 0 or above iterations."""
    b = np.ascontiguousarray(np.asarray(budgets).astype(np.uint32)).reshape(-1)
    _lib.check(_lib.load().oakgpu_forest_budgets_check(b.ctypes.data_as(C.c_void_p) if len(b) else None, len(b), int(iterations)))
