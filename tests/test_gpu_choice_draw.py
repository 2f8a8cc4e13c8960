"""The random policy's pick of one legal choice per side (EngineR::legal, nth_choice and the draws of random_choices) against the CPU
oracle: exactly ONE turn-step of states edited so that every shape of a choice list occurs for each player -- every set of live bench
Pokemon, every set of move slots without PP, a disabled slot, empty trailing slots, the forced moves (recharging, Rage, thrashing,
charging, Bide and binding with the selected move in each slot and in none) and the switch / pass requests after a faint -- under
several choice-stream seeds each, so that every (length of the list, index drawn) occurs for P1 (seed % m on 64 bits) and for P2
((seed >> 32) % n).  The preconditions are checked on the oracle's side alone, without a GPU.  A second case plays one group of
3 x 2,048 playouts to the end.

The launches are small and run with the lane spread off (oakgpu_set_spread 0), like tests/test_gpu_move_carry.py's."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
from inert_ref import ACTIVE, LAST_SEL, ORDER, SIDE, V, u16

SEEDS = 6
KEYS = ("results", "steps", "prng", "battles", "durations")
PASS, MOVE, SWITCH = 0, 1, 2
MOVING, ERROR = 0x50, 4
FORCED = V["RECHARGING"] | V["RAGE"] | V["THRASHING"] | V["CHARGING"] | V["BIDE"] | V["BINDING"]
# the lock and the move that causes it: (volatile, selected move, does an attack counter run)
LOCKS = {"recharging": (V["RECHARGING"], 63, False), "rage": (V["RAGE"], 99, False), "thrashing": (V["THRASHING"], 37, True),
         "charging": (V["CHARGING"], 76, False)}
LIMITS = {"bide": (V["BIDE"], 117), "binding": (V["BINDING"], 35)}


def _stored(b, s, pos):
    return s * SIDE + (int(b[s * SIDE + ORDER + pos]) - 1) * 24


def _vlo(b, s):
    o = s * SIDE + ACTIVE + 16
    return int(b[o]) | int(b[o + 1]) << 8 | int(b[o + 2]) << 16 | int(b[o + 3]) << 24


def _set_vlo(b, s, v):
    o = s * SIDE + ACTIVE + 16
    b[o:o + 4] = [(v >> (8 * k)) & 0xFF for k in range(4)]


def _set_bench(b, s, alive):
    """Bit p - 1 of `alive`: the Pokemon at party position p + 1 lives (a fainted one has no HP and no status)."""
    for pos in range(1, 6):
        o = _stored(b, s, pos)
        if (alive >> (pos - 1)) & 1:
            if u16(b, o + 18) == 0:
                b[o + 18:o + 20] = b[o:o + 2]
        else:
            b[o + 18:o + 21] = 0


def _set_move(b, s, i, mid=None, pp=None):
    """Move slot i of the active Pokemon and of its party entry (the two agree unless a Transform or Mimic stands between them)."""
    for o in (s * SIDE + ACTIVE + 24 + 2 * i, _stored(b, s, 0) + 10 + 2 * i):
        if mid is not None:
            b[o] = mid
        if pp is not None:
            b[o + 1] = pp


def _disable(b, d, s, slot):
    o = s * SIDE + ACTIVE
    b[o + 22] = (b[o + 22] & 0x0F) | (3 << 4)        # 3 turns left ...
    b[o + 23] = (b[o + 23] & 0xF8) | slot            # ... on this move slot
    w = d.view(np.uint32)
    w[s] = (w[s] & ~np.uint32(15 << 21)) | np.uint32(1 << 21)


def _lock(b, s, bit, sel, counter):
    v = _vlo(b, s) | bit
    if counter:
        v = (v & ~(7 << 21)) | (2 << 21)             # two more attacks
    _set_vlo(b, s, v)
    b[s * SIDE + LAST_SEL] = sel


@functools.lru_cache(maxsize=None)
def _bases():
    """Random OU battles a few turn-steps in: (those where both sides choose freely among four moves, those that ask for a switch)."""
    b, d, p, r = O.make_random_ou_batch(1536, seed0=0x22CD00000000)
    res = np.zeros(len(b), dtype=np.uint8)
    for k, steps in enumerate((3, 5, 8, 12, 17, 23)):
        sl = slice(256 * k, 256 * (k + 1))
        res[sl], _ = O.rollout_batch(b[sl], d[sl], r[sl], p[sl], max_steps=steps, threads=4)
    free, asked = [], []
    for k in range(len(b)):
        if res[k] in (0x20, 0x80, 0xA0):
            asked.append(k)
        plain = all((_vlo(b[k], s) & (FORCED | V["TRANSFORM"])) == 0 and (b[k, s * SIDE + ACTIVE + 23] & 7) == 0 and
                    all(b[k, s * SIDE + ACTIVE + 24 + 2 * i] != 0 and b[k, s * SIDE + ACTIVE + 25 + 2 * i] != 0 for i in range(4)) and
                    u16(b[k], _stored(b[k], s, 0) + 18) > 0 for s in range(2))
        if res[k] == MOVING and plain:
            free.append(k)
    assert len(free) >= 64 and len(asked) >= 16, (len(free), len(asked))
    return b, d, res, tuple(free), tuple(asked)


@functools.lru_cache(maxsize=None)
def _states():
    """(battles, durations, results, tag of each state): the edited states, one row each."""
    base_b, base_d, base_r, free, asked = _bases()
    rows, tags, take = [], [], [0]

    def fresh(pool=free):
        k = pool[take[0] % len(pool)]
        take[0] += 1
        return base_b[k].copy(), base_d[k].copy(), int(base_r[k])

    def add(tag, b, d, r):
        rows.append((b, d, r))
        tags.append(tag)

    for s in range(2):
        for alive in range(32):                      # every set of live bench Pokemon x every set of move slots without PP
            for empty in range(16):
                b, d, r = fresh()
                _set_bench(b, s, alive)
                for i in range(4):
                    if (empty >> i) & 1:
                        _set_move(b, s, i, pp=0)
                add("bench x pp", b, d, r)
        for slot in range(5):                        # a disabled slot (0: none) x every set of move slots without PP
            for empty in range(16):
                b, d, r = fresh()
                if slot:
                    _disable(b, d, s, slot)
                for i in range(4):
                    if (empty >> i) & 1:
                        _set_move(b, s, i, pp=0)
                add("disabled %d" % slot, b, d, r)
        for first in range(1, 4):                    # empty trailing slots, with and without PP left in them, one with PP in front empty too
            for keep_pp in (False, True):
                for front_empty in (False, True):
                    b, d, r = fresh()
                    for i in range(first, 4):
                        _set_move(b, s, i, mid=0, pp=None if keep_pp else 0)
                    if front_empty:
                        _set_move(b, s, 0, pp=0)
                    add("trailing", b, d, r)
        b, d, r = fresh()                            # an empty slot in FRONT of a move: the list ends at the first empty slot
        _set_move(b, s, 1, mid=0)
        add("trailing", b, d, r)
        for name, (bit, sel, counter) in LOCKS.items():
            for _ in range(2):
                b, d, r = fresh()
                _lock(b, s, bit, sel, counter)
                add(name, b, d, r)
        for name, (bit, sel) in LIMITS.items():
            for slot in range(5):                    # the selected move in each slot; 4: in none
                b, d, r = fresh()
                for i in range(4):
                    if b[s * SIDE + ACTIVE + 24 + 2 * i] == sel:
                        _set_move(b, s, i, mid=1)    # (Pound: the selected move stands where the case puts it and nowhere else)
                if slot < 4:
                    _set_move(b, s, slot, mid=sel)
                _lock(b, s, bit, sel, True)
                add("%s %d" % (name, slot), b, d, r)
    for alive in range(1, 32):                       # after a faint: the switch request with every set of live bench Pokemon, and the pass
        b, d, r = fresh(asked)
        for s in range(2):
            if ((r >> (4 + 2 * s)) & 3) == SWITCH:
                _set_bench(b, s, alive)
        add("after a faint %02x" % r, b, d, r)
    b = np.stack([x[0] for x in rows])
    d = np.stack([x[1] for x in rows])
    r = np.array([x[2] for x in rows], dtype=np.uint8)
    return b, d, r, tuple(tags)


@functools.lru_cache(maxsize=None)
def _cases():
    """Every state under SEEDS choice streams, and the oracle's turn-step of each (computed once, read-only)."""
    b, d, r, tags = _states()
    b, d, r = np.repeat(b, SEEDS, axis=0), np.repeat(d, SEEDS, axis=0), np.repeat(r, SEEDS)
    p = np.zeros((len(b), 8), dtype=np.uint8)
    O.LIB.oracle_fast_prng_seed_batch(O.ptr(p), len(p), C.c_uint64(0x22C0FFEE0000))
    ob, od, op = b.copy(), d.copy(), p.copy()
    oout, osteps = O.rollout_batch(ob, od, r, op, max_steps=1, threads=8)
    exp = dict(results=oout, steps=osteps, prng=op, battles=ob, durations=od)
    for a in (b, d, r, p) + tuple(exp.values()):
        a.setflags(write=False)
    return b, d, r, p, exp, tuple(t for t in tags for _ in range(SEEDS))


def _draws():
    """(list length, index drawn) of each case, per player, by the oracle's own choices and generator."""
    b, d, r, p, _, _ = _cases()
    out = np.zeros((len(b), 2, 2), dtype=np.int64)
    for k in range(len(b)):
        seed = O.LIB.oracle_fast_prng_uniform_64(O.ptr(p[k].copy()))
        m, n = len(O.choices(b[k], 0, (int(r[k]) >> 4) & 3)), len(O.choices(b[k], 1, (int(r[k]) >> 6) & 3))
        out[k] = ((m, seed % m), (n, (seed >> 32) % n))
    return out


def test_the_cases_cover_every_list_length_and_index_and_the_oracle_accepts_them():
    b, d, r, p, exp, tags = _cases()
    draws = _draws()
    for player in range(2):
        seen = {(int(n), int(i)) for n, i in draws[:, player]}
        missing = [(n, i) for n in range(1, 10) for i in range(n) if (n, i) not in seen]
        assert not missing, ("P%d never draws" % (player + 1), missing)
    assert ((exp["results"] & 15) != ERROR).all(), sorted({tags[k] for k in np.where((exp["results"] & 15) == ERROR)[0]})
    assert (exp["steps"] == 1).all()
    want = {"bench x pp", "trailing"} | {"disabled %d" % k for k in range(5)} | set(LOCKS) | {"%s %d" % (n, k) for n in LIMITS for k in range(5)}
    assert want <= set(tags) and {"after a faint 20", "after a faint 80"} <= set(tags), sorted(set(tags))
    # the edits did what they say: a forced side has one choice, a side that is asked to switch as many as it has live bench Pokemon
    for k in range(0, len(b), SEEDS):
        forced = [s for s in range(2) if _vlo(b[k], s) & FORCED and ((int(r[k]) >> (4 + 2 * s)) & 3) == MOVE]
        assert all(draws[k, s, 0] == 1 for s in forced), tags[k]


def _compare(got, exp, tags, what):
    bad = np.zeros(len(tags), dtype=bool)
    for key in KEYS:
        ne = got[key] != exp[key]
        bad |= ne if ne.ndim == 1 else ne.any(axis=1)
    assert not bad.any(), (what, int(bad.sum()), sorted({tags[k] for k in np.where(bad)[0]}))


def _spread(ctx, lanes):
    from oak_amd import _lib
    _lib.check(ctx.lib.oakgpu_set_spread(ctx.handle, lanes))


@pytest.fixture
def ctx(gpu_ctx):
    """The session's context with no lane spread; the schedule settings back to their defaults afterwards."""
    from test_gpu_move_carry import DEFAULT
    _spread(gpu_ctx, 0)
    try:
        yield gpu_ctx
    finally:
        _spread(gpu_ctx, -1)
        gpu_ctx.set_playouts_per_lane(2)
        gpu_ctx.set_move_carry(DEFAULT)


@pytest.mark.gpu
def test_one_turn_step_of_every_case_through_the_group_launch(ctx):
    b, d, r, p, exp, tags = _cases()
    got = ctx.rollout_group([(b, d, r, p)], max_steps=1, return_state=True)[0]
    _compare(got, exp, tags, "rollout_group")


@pytest.mark.gpu
def test_one_turn_step_of_every_case_through_rollout_dev(ctx):
    from hipmem import Dev
    from oak_amd import _lib
    b, d, r, p, exp, tags = _cases()
    n = len(b)
    dev = {"b": Dev(b), "d": Dev(d), "r": Dev(r), "p": Dev(p), "ro": Dev(r, fill=0), "st": Dev(np.zeros(n, dtype=np.uint32), fill=0),
           "va": Dev(np.zeros(n, dtype=np.float32), fill=0), "bo": Dev(b, fill=0), "do": Dev(d, fill=0)}
    try:
        _lib.check(ctx.lib.oakgpu_rollout_dev(ctx.handle, dev["b"].p, dev["d"].p, dev["r"].p, dev["p"].p, n, 1, 0, dev["ro"].p, dev["st"].p,
                                              dev["va"].p, dev["bo"].p, dev["do"].p))
        ctx.synchronize()
        got = dict(results=dev["ro"].host(), steps=dev["st"].host(), prng=dev["p"].host(), battles=dev["bo"].host(), durations=dev["do"].host())
    finally:
        for x in dev.values():
            x.free()
    _compare(got, exp, tags, "oakgpu_rollout_dev")


@functools.lru_cache(maxsize=None)
def _group():
    out = []
    for k in range(3):
        b, d, p, r = O.make_random_ou_batch(2048, seed0=0x22CE00000000 + 2048 * k)
        ob, od, op = b.copy(), d.copy(), p.copy()
        oout, osteps = O.rollout_batch(ob, od, r, op, max_steps=1000, threads=8)
        exp = dict(results=oout, steps=osteps, prng=op, battles=ob, durations=od)
        for a in (b, d, p, r) + tuple(exp.values()):
            a.setflags(write=False)
        out.append(((b, d, r, p), exp))
    return tuple(out)


@pytest.mark.gpu
def test_a_group_of_three_batches_to_the_end_with_and_without_the_move_carry(ctx):
    from test_gpu_move_carry import DEFAULT
    ctx.set_playouts_per_lane(4)
    for below in sorted({0, DEFAULT}):
        ctx.set_move_carry(below)
        got = ctx.rollout_group([batch for batch, _ in _group()], max_steps=1000, return_state=True)
        for k, (g, (_, exp)) in enumerate(zip(got, _group())):
            _compare(g, exp, ("batch %d" % k,) * len(exp["steps"]), (below, k))
        assert ctx.queue_counters()[63] == 0
