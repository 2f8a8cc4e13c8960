"""CPU: tests/forest_ref.py's numpy restatement of the UCB / PUCB bandits equals oak_amd/csrc/bandit.hpp bit for bit (through the host-only
oakgpu_bandit_replay), and its replayer accepts a consistent tree trace and rejects one with a selection or a value altered.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import forest_ref as R

F = np.float32


def _lib():
    import __graft_entry__ as g
    g.build()
    from oak_amd import _lib
    return _lib, _lib.load()


def _replay(lib, kind, c, k, logits, values):
    steps = len(values)
    idx, stats, visits = np.zeros(max(steps, 1), np.uint8), np.zeros(18, F), np.zeros(9, np.uint32)
    v = np.ascontiguousarray(values, F) if steps else np.zeros(1, F)
    lg = np.ascontiguousarray(logits, F) if logits is not None else None
    rc = lib.oakgpu_bandit_replay(kind, C.c_float(c), C.c_float(0.0), k, lg.ctypes.data_as(C.c_void_p) if lg is not None else None, steps, None,
                                  v.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), None, stats.ctypes.data_as(C.c_void_p),
                                  visits.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return idx[:steps], stats[:9].copy(), stats[9:].copy(), visits


@pytest.mark.parametrize("kind", [R.UCB, R.PUCB])
@pytest.mark.parametrize("k", range(1, 10))
def test_restatement_equals_bandit_hpp_bit_for_bit(kind, k):
    _, lib = _lib()
    rng = np.random.default_rng(1000 * kind + k)
    for c in (1.0, 2.0, 0.37):
        steps = 300
        # values of every kind a search backs up: exact 0 / 0.5 / 1 and arbitrary floats, so that ties and near-ties between arms occur
        values = np.where(rng.random(steps) < 0.5, rng.choice([0.0, 0.5, 1.0], steps), rng.random(steps)).astype(F)
        logits = (rng.standard_normal(9) * 3).astype(F) if kind == R.PUCB else None
        _, _, priors, _ = _replay(lib, kind, c, k, logits, [])   # the priors as bandit.hpp wrote them
        if kind == R.PUCB:
            R.check_priors(priors, k, kind, logits, "host priors")
        b = R.Bandit()
        b.init(k)
        b.priors[:] = priors
        got = []
        for t in range(steps):
            i = b.select(kind, c)
            b.visit(i)
            b.update(i, values[t])
            got.append(i)
        idx, scores, pr, visits = _replay(lib, kind, c, k, logits, values)
        assert got == [int(x) for x in idx]
        assert b.same_as(k, scores, pr, visits)


def _toy_tree(seed, iterations, kind, c, max_depth):
    """A tree grown by the restatement over a random environment, in the forest search's iteration order: (trace, final node records, root logits)."""
    from oak_amd.search import trace_dtype
    rng = np.random.default_rng(seed)
    trace = np.zeros(iterations, dtype=trace_dtype(max_depth))

    def new_node():
        nd = [R.Bandit(), R.Bandit()]
        lg = (rng.standard_normal((2, 9)) * 2).astype(F)
        for s in range(2):
            nd[s].init(int(rng.integers(1, 4)))
            if kind == R.PUCB:
                y = np.exp(lg[s, :nd[s].k])
                nd[s].priors[:nd[s].k] = (y / F(sum(y, F(0)))).astype(F)
        return nd, lg

    root, root_lg = new_node()
    nodes, edges = [root], {}
    for t in range(iterations):
        rec, cur, d = trace[t], 0, 0
        rec["leaf"] = R.NO_NODE
        while True:
            nd = nodes[cur]
            i, j = nd[0].select(kind, c), nd[1].select(kind, c)
            nd[0].visit(i)
            nd[1].visit(j)
            rec["path"][d] = (cur, i, j, (0, 0))
            d += 1
            if rng.random() < 0.08:
                rec["result_type"] = int(rng.integers(1, 4))
                rec["value"] = R.value_of_result(int(rec["result_type"]))
                break
            key = (cur, i, j, int(rng.integers(0, 2)))
            if key not in edges:
                edges[key] = len(nodes)
                nodes.append(None)
            child = edges[key]
            if nodes[child] is not None and d < max_depth:
                cur = child
                continue
            rec["leaf"], rec["value"] = child, F(rng.random())
            if nodes[child] is None:
                nodes[child], lg = new_node()
                rec["initialised"] = 1
                if kind == R.PUCB:
                    rec["logits"] = lg
            break
        rec["levels"] = d
        for q in range(d):
            nd = nodes[int(rec["path"][q]["node"])]
            nd[0].update(int(rec["path"][q]["i"]), rec["value"])
            nd[1].update(int(rec["path"][q]["j"]), F(1.0) - F(rec["value"]))
    records = [tuple((b.k, b.scores.copy(), b.priors.copy(), b.visits.copy()) for b in nd) for nd in nodes]
    return trace, records, (root_lg if kind == R.PUCB else None)


@pytest.mark.parametrize("kind", [R.UCB, R.PUCB])
def test_replayer_accepts_a_consistent_trace_and_rejects_altered_ones(kind):
    _lib()
    trace, nodes, root_lg = _toy_tree(7 + kind, 200, kind, 1.0, 3)
    cover = R.replay(trace, nodes, kind, 1.0, 3, root_lg)
    assert cover["terminal"] and cover["deep"] and cover["capped"] and cover["k1"]
    # one selection altered: an iteration at a node with a choice takes another arm
    bad = trace.copy()
    t = next(q for q in range(50, 200) if nodes[int(bad[q]["path"][0]["node"])][0][0] > 1)
    bad[t]["path"][0]["i"] = (int(bad[t]["path"][0]["i"]) + 1) % nodes[0][0][0]
    with pytest.raises(AssertionError, match="traced selection"):
        R.replay(bad, nodes, kind, 1.0, 3, root_lg)
    # one value altered, at an evaluated leaf (the final statistics no longer follow) and at a terminal edge
    bad = trace.copy()
    t = next(q for q in range(200) if int(bad[q]["leaf"]) != R.NO_NODE)
    bad[t]["value"] = F(bad[t]["value"]) + F(0.125)
    with pytest.raises(AssertionError):
        R.replay(bad, nodes, kind, 1.0, 3, root_lg)
    bad = trace.copy()
    t = next(q for q in range(200) if int(bad[q]["leaf"]) == R.NO_NODE)
    bad[t]["value"] = F(0.25)
    with pytest.raises(AssertionError, match="terminal value"):
        R.replay(bad, nodes, kind, 1.0, 3, root_lg)
    # a prior outside the bound
    if kind == R.PUCB:
        k = nodes[0][0][0]
        off = [tuple((s[0], s[1], s[2].copy(), s[3]) for s in nd) for nd in nodes]
        off[0][0][2][0] *= F(1.0 + 64 * 2.0 ** -24)
        if k > 1:
            with pytest.raises(AssertionError, match="prior off"):
                R.replay(trace, off, kind, 1.0, 3, root_lg)
