"""Back-to-back group launches on two streams ("the other stream"): the adoption tickets are tagged with a per-context
launch epoch instead of being cleared by every launch, the launch's control words are cleared by its own first kernel, k_queue_order
runs in 256-thread blocks.  None of it may change a byte: everything here is held to the CPU oracle, which knows nothing of queues."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

KEYS = ("results", "steps", "values", "battles", "durations", "prng")
SPLITS = {8192: (3000, 5000, 192), 20000: (7001, 12000, 999)}   # one group of three uneven batches
N = 20000


class Case:
    """20,000 random OU playouts and what the oracle makes of them (cap 1,000); playouts are independent, so the first 8,192 of
    them are the 8,192-playout case."""

    def __init__(self, seed0):
        self.b, self.d, self.p, self.r = O.make_random_ou_batch(N, seed0=seed0)
        self.ob, self.od, self.op = self.b.copy(), self.d.copy(), self.p.copy()
        self.oout, self.osteps = O.rollout_batch(self.ob, self.od, self.r, self.op, max_steps=1000, threads=8)
        t = self.oout & 15
        self.ovalues = np.where(t == 1, 1.0, np.where(t == 2, 0.0, 0.5)).astype(np.float32)

    def batches(self, total):
        out, o = [], 0
        for n in SPLITS[total]:
            out.append((self.b[o:o + n], self.d[o:o + n], self.r[o:o + n], self.p[o:o + n]))
            o += n
        return out

    def expected(self, total):
        return dict(results=self.oout[:total], steps=self.osteps[:total], values=self.ovalues[:total], battles=self.ob[:total],
                    durations=self.od[:total], prng=self.op[:total])


@pytest.fixture(scope="module")
def case_a():
    return Case(0x15A00000000)


@pytest.fixture(scope="module")
def case_b():
    return Case(0x15B00000000)


def _joined(outs):
    return {k: np.concatenate([o[k] for o in outs]) for k in KEYS}


def _force(ctx):
    ctx.set_playouts_per_lane(2)
    ctx.set_migration(2, 120, 8)     # always; donate what still runs after 120 turn-steps to 8 adopter waves
    ctx.set_migration_window(24)


def _defaults(ctx):
    ctx.set_migration(1, 300, 0)
    ctx.set_migration_window(48)


def _check(got, exp, what):
    for k in KEYS:
        bad = np.nonzero((got[k] != exp[k]).reshape(len(exp[k]), -1).any(axis=1))[0]
        assert bad.size == 0, (what, k, "first differing playout", int(bad[0]), "of", int(bad.size))


@pytest.mark.parametrize("total", [8192, 20000])
def test_tagged_tickets_bit_exact(gpu_ctx, case_a, total):
    """Migration always, queue order on: every output byte is the oracle's, no bounded wait ran out, and playouts
    really travelled through the tagged tickets."""
    _force(gpu_ctx)
    try:
        got = _joined(gpu_ctx.rollout_group(case_a.batches(total), max_steps=1000, return_state=True))
        c = gpu_ctx.queue_counters()
        assert c[63] == 0, ("bounded wait ran out", int(c[63]))
        assert c[40] > 0 and c[40] == c[41], ("donations / adoptions", int(c[40]), int(c[41]))
        assert c[32] + c[33] + c[34] + c[35] == total, "the queue order ran"
        _check(got, case_a.expected(total), total)
    finally:
        _defaults(gpu_ctx)


def test_epoch_reuse_three_launches_without_clearing(gpu_ctx, case_a):
    """The same launch three times on one context: the second and third find the first one's tickets in the list (another epoch)
    and must not take them for their own."""
    _force(gpu_ctx)
    try:
        first = None
        for rep in range(3):
            got = _joined(gpu_ctx.rollout_group(case_a.batches(20000), max_steps=1000, return_state=True))
            c = gpu_ctx.queue_counters()
            assert c[63] == 0 and c[40] > 0 and c[40] == c[41], (rep, int(c[63]), int(c[40]), int(c[41]))
            if first is None:
                first = got
                _check(got, case_a.expected(20000), "first launch")
            else:
                _check(got, first, "launch %d against the first" % rep)
    finally:
        _defaults(gpu_ctx)


def test_two_contexts_launch_at_once(gpu_ctx, case_a, case_b):
    """Two contexts launch at the same time on their own streams, twice: both are bit-identical to what
    each computes alone (= the oracle's bytes; the second launch continues the first one's choice streams)."""
    from hipmem import Dev
    from oak_amd import _lib
    from oak_amd.engine import Context
    other = Context(0)
    runs = []
    try:
        for ctx, case in ((gpu_ctx, case_a), (other, case_b)):
            _force(ctx)
            dev = {"b": Dev(case.b), "d": Dev(case.d), "p": Dev(case.p), "r": Dev(case.r), "ro": Dev(case.r, fill=0),
                   "st": Dev(np.zeros(N, dtype=np.uint32)), "va": Dev(np.zeros(N, dtype=np.float32)), "bo": Dev(case.b, fill=0), "do": Dev(case.d, fill=0)}
            batches = (_lib.RolloutBatch * 3)()
            o = 0
            for j, n in enumerate(SPLITS[N]):
                at = lambda key, stride: C.c_void_p(dev[key].p.value + o * stride)
                batches[j] = _lib.RolloutBatch(at("b", 384), at("d", 8), at("r", 1), at("p", 8), n, at("ro", 1), at("st", 4), at("va", 4), at("bo", 384), at("do", 8))
                o += n
            runs.append((ctx, case, dev, batches))
        for rep in range(2):
            for ctx, case, dev, batches in runs:
                _lib.check(ctx.lib.oakgpu_rollout_group_dev(ctx.handle, batches, 3, 1000, 0))
        for ctx, case, dev, batches in runs:
            c = ctx.queue_counters()              # synchronises the context's stream
            assert c[63] == 0 and c[40] > 0 and c[40] == c[41], (int(c[63]), int(c[40]), int(c[41]))
            ob, od = case.b.copy(), case.d.copy()
            op = case.op.copy()                   # the choice streams where the first launch left them
            oout, osteps = O.rollout_batch(ob, od, case.r, op, max_steps=1000, threads=8)
            assert (dev["ro"].host() == oout).all() and (dev["st"].host() == osteps).all()
            assert (dev["bo"].host() == ob).all() and (dev["do"].host() == od).all() and (dev["p"].host() == op).all()
            t = oout & 15
            assert (dev["va"].host() == np.where(t == 1, 1.0, np.where(t == 2, 0.0, 0.5)).astype(np.float32)).all()
    finally:
        for ctx, case, dev, batches in runs:
            try:
                ctx.synchronize()
            except Exception:
                pass
            for x in dev.values():
                x.free()
        _defaults(gpu_ctx)
        other.close()


def _suspects(battles):
    """k_queue_order's predicate: a Ghost type or a Ditto among the twelve Pokemon (side s at 184 s, Pokemon k at + 24 k; species byte
    21, types byte 22)."""
    s = np.zeros(len(battles), dtype=bool)
    for side in range(2):
        for k in range(6):
            o = side * 184 + k * 24
            sp, ty = battles[:, o + 21], battles[:, o + 22]
            s |= (sp != 0) & (((ty & 15) == 7) | ((ty >> 4) == 7) | (sp == 132))
    return s


@pytest.mark.parametrize("total", [8191, 8193])
@pytest.mark.parametrize("nbatch", [1, 3])
def test_queue_order_256_thread_blocks(gpu_ctx, case_a, total, nbatch):
    """The order is a permutation of 0 .. total - 1 with every suspect in front of every other playout (sizes one short of and one
    past eight full 1,024-playout blocks; batch borders inside a block)."""
    cuts = [0, total] if nbatch == 1 else [0, 1000, 1000 + 4097, total]
    parts = [case_a.b[cuts[i]:cuts[i + 1]] for i in range(nbatch)]
    order, n_suspects = gpu_ctx.queue_order(parts)
    assert (np.sort(order) == np.arange(total, dtype=np.uint32)).all(), "not a permutation"
    s = _suspects(case_a.b[:total])
    assert n_suspects == int(s.sum())
    assert s[order[:n_suspects]].all() and not s[order[n_suspects:]].any()
