"""The UCB / PUCB bandits of oak_amd/csrc/bandit.hpp restated in numpy float32 (init / select / visit / update, statement for
statement), and a replayer that holds one tree of the forest search (oak_amd/csrc/forest.hip) to its own trace.

The restatement is pinned to bandit.hpp bit for bit by tests/test_forest_ref.py (through oakgpu_bandit_replay, no GPU).  The replayer
takes a tree's trace (one record per iteration: the path's (node, i, j), the leaf, the value backed up, a new PUCB node's logits) and
the tree's final node records, walks every iteration from the root and checks
  1. every traced (i, j) is what select returns on the statistics at that moment;
  2. every node's priors against the float64 softmax of its traced logits, relative error <= PRIOR_BOUND = 16 x 2^-24: expf is good
     to 1 ulp (2^-23 relative at worst = 2 x 2^-24), the fp32 sum of <= 9 terms rounds <= 8 times (8 x 2^-24), the quotient once
     (2^-24), and the float64 reference's own error is far below; 13 x 2^-24, rounded up.  UCB nodes hold exactly 1 / k;
  3. after visit and update along every path, the final statistics equal the device's node records bit for bit.
Priors (and a node's k) are taken AS THE DEVICE WROTE THEM: the device's expf is not the host's, so they are bounded (2), not
recomputed."""
import numpy as np

F = np.float32
UCB, PUCB = 0, 1
NO_NODE = 0xFFFFFFFF
PRIOR_BOUND = 16 * 2.0 ** -24


class Bandit:
    """oak_search::Bandit for the counting kinds UCB and PUCB."""

    def __init__(self):
        self.k = 0
        self.scores = np.zeros(9, F)
        self.priors = np.zeros(9, F)
        self.visits = np.zeros(9, np.uint32)

    def init(self, k):
        self.k = int(k)
        self.priors[:] = F(1.0) / F(k) if k else F(0.0)
        self.scores[:] = F(0.5)
        self.visits[:] = 1

    def select(self, kind, c):
        k = self.k
        if k == 1:
            return 0
        N = int(self.visits[:k].astype(np.uint64).sum())
        sqrtN = F(np.sqrt(np.float64(N)))
        c = F(c)
        best, idx = F(0.0), 0
        for i in range(k):
            e = F(c * self.priors[i]) * sqrtN if kind == PUCB else F(c * sqrtN) / F(k)
            a = F(e + self.scores[i]) / F(self.visits[i])
            if a > best:
                best, idx = a, i
        return idx

    def visit(self, i):
        self.visits[i] += np.uint32(1)

    def update(self, i, value):
        self.scores[i] = F(self.scores[i] + F(value))

    def same_as(self, k, scores, priors, visits):
        return (self.k == k and self.scores.tobytes() == np.asarray(scores, F).tobytes() and self.priors.tobytes() == np.asarray(priors, F).tobytes()
                and self.visits.tobytes() == np.asarray(visits, np.uint32).tobytes())


def softmax64(logits):
    y = np.exp(np.asarray(logits, np.float64))
    return y / y.sum()


def check_priors(priors, k, kind, logits, where):
    priors = np.asarray(priors, F)
    if kind == UCB or logits is None:
        want = F(1.0) / F(k)
        assert (priors == want).all(), "%s: UCB priors are not 1 / k" % where
        return
    want = softmax64(np.asarray(logits, np.float64)[:k])
    err = np.abs(priors[:k].astype(np.float64) - want) / want
    assert err.max() <= PRIOR_BOUND, "%s: prior off the float64 softmax of its logits by %.3g relative (bound %.3g)" % (where, err.max(), PRIOR_BOUND)


class _Node:
    def __init__(self, record):
        (k1, _, pr1, _), (k2, _, pr2, _) = record
        self.p1, self.p2 = Bandit(), Bandit()
        self.p1.init(k1)
        self.p2.init(k2)
        self.p1.priors[:] = np.asarray(pr1, F)   # as the device wrote them
        self.p2.priors[:] = np.asarray(pr2, F)


def value_of_result(t):
    return F(1.0) if t == 1 else F(0.0) if t == 2 else F(0.5)


def replay(trace, nodes, kind, c, max_depth, root_logits=None):
    """Holds one tree to its trace.  trace: iterable of records with fields levels, leaf, initialised, result_type, value, logits [2, 9],
    path [levels] of (node, i, j); nodes: the final records [((k, scores, priors, visits) of p1, of p2), ...] in creation order;
    root_logits: None or (p1 logits, p2 logits).  Raises AssertionError naming the first disagreement; returns the coverage counts
    {"terminal", "deep" (>= 3 levels), "k1" (nodes with a single action on a side), "capped" (stopped by max_depth on an initialised node)}."""
    max_depth = max_depth if max_depth else 100
    assert len(nodes) >= 1 and nodes[0][0][0] > 0 and nodes[0][1][0] > 0, "the root is not initialised"
    tree = [_Node(nodes[0])]
    check_priors(nodes[0][0][2], nodes[0][0][0], kind, None if root_logits is None else root_logits[0], "root p1")
    check_priors(nodes[0][1][2], nodes[0][1][0], kind, None if root_logits is None else root_logits[1], "root p2")
    cover = {"terminal": 0, "deep": 0, "k1": 0, "capped": 0}
    for t, rec in enumerate(trace):
        L = int(rec["levels"])
        assert 1 <= L <= max_depth, "iteration %d: %d levels" % (t, L)
        v1 = F(rec["value"])
        for d in range(L):
            nid = int(rec["path"][d]["node"])
            assert nid < len(tree), "iteration %d level %d: node %d does not exist yet" % (t, d, nid)
            assert d > 0 or nid == 0, "iteration %d: the walk does not start at the root" % t
            nd = tree[nid]
            i, j = nd.p1.select(kind, c), nd.p2.select(kind, c)
            got = (int(rec["path"][d]["i"]), int(rec["path"][d]["j"]))
            assert (i, j) == got, "iteration %d level %d node %d: traced selection %s, select gives %s" % (t, d, nid, got, (i, j))
            nd.p1.visit(i)
            nd.p2.visit(j)
        leaf, rt = int(rec["leaf"]), int(rec["result_type"])
        if leaf == NO_NODE:
            assert rt != 0 and not rec["initialised"], "iteration %d: no leaf without a terminal edge" % t
            assert v1 == value_of_result(rt), "iteration %d: terminal value %r for result type %d" % (t, v1, rt)
            cover["terminal"] += 1
        else:
            assert rt == 0, "iteration %d: a leaf behind a terminal edge" % t
            if rec["initialised"]:
                assert leaf == len(tree), "iteration %d: new node %d is not the next in creation order (%d)" % (t, leaf, len(tree))
                assert leaf < len(nodes), "iteration %d: node %d has no record" % (t, leaf)
                tree.append(_Node(nodes[leaf]))
                lg = np.asarray(rec["logits"], F).reshape(2, 9) if kind == PUCB else (None, None)
                check_priors(nodes[leaf][0][2], nodes[leaf][0][0], kind, lg[0], "node %d p1" % leaf)
                check_priors(nodes[leaf][1][2], nodes[leaf][1][0], kind, lg[1], "node %d p2" % leaf)
            else:
                assert leaf < len(tree) and L == max_depth, "iteration %d: stopped at the initialised node %d above the depth cap" % (t, leaf)
                cover["capped"] += 1
        cover["deep"] += L >= 3
        for d in range(L):
            nd = tree[int(rec["path"][d]["node"])]
            nd.p1.update(int(rec["path"][d]["i"]), v1)
            nd.p2.update(int(rec["path"][d]["j"]), F(1.0) - v1)
    assert len(tree) == len(nodes), "the trace creates %d nodes, the tree holds %d" % (len(tree), len(nodes))
    for q, (nd, record) in enumerate(zip(tree, nodes)):
        assert nd.p1.same_as(*record[0]) and nd.p2.same_as(*record[1]), "node %d: the replayed statistics differ from the tree's" % q
        cover["k1"] += record[0][0] == 1 or record[1][0] == 1
    return cover
