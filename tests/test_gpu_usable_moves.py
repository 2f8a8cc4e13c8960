"""Which move slots a side may choose from (EngineR::legal, oak_amd/csrc/gen1_regs.hpp: a move, PP, not disabled, no empty slot in front)
as the moves, their PP and the disabled slot CHANGE over a game.  Edited states are played under step caps 1 .. 12 and compared with the
CPU oracle at EVERY cap, byte for byte, so that each change happens and a later turn's legal() has to see it:

  pp         every subset of a side's slots at 1 PP, nobody to switch to: the list shrinks as moves are used, down to Struggle
  disable    the foe knows nothing but Disable: it lands on one slot or another and runs out
  haze       a slot is disabled and the foe, or the side itself, knows nothing but Haze
  mimic      Mimic in each slot with its last PP (the copied move cannot be chosen) and with PP to spare (it can)
  transform  Transform against a foe whose trailing slots are empty, with a bench to switch out to and come back from
  empty      a switch to a Pokemon that has no PP left: Struggle from the first turn on

through k_rollout_queue with the move carry on and off, as tests/test_gpu_move_carry.py does, and through k_root_step in slices of 4
turn-steps, where a playout's registers cross from launch to launch.  (Written for a cached form of that list, which lost on the
counters and was taken out again -- profiles/r31_engine_diet.json; whoever caches it next has the cases.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
from inert_ref import ACTIVE, LAST_USED, ORDER, SIDE, V, u32
from oak_amd import gamedata
from test_gpu_choice_draw import _bases, _compare, _disable, _set_bench, _set_move, _spread, _stored, _vlo

SEEDS, CAPS = 4, range(1, 13)
DISABLE, HAZE, MIMIC, TRANSFORM, STRUGGLE = (gamedata.MOVE_NAMES.index(n) for n in ("Disable", "Haze", "Mimic", "Transform", "Struggle"))


def _all_slots(b, s, mid, pp):
    for i in range(4):
        _set_move(b, s, i, mid=mid, pp=pp)


def _bench_without_pp(b, s):
    """Only party position 2 lives, and none of its moves has PP."""
    _set_bench(b, s, 1)
    o = _stored(b, s, 1)
    for i in range(4):
        b[o + 11 + 2 * i] = 0


@functools.lru_cache(maxsize=None)
def _states():
    base_b, base_d, base_r, free, _ = _bases()
    rows, tags, take = [], [], [0]

    def fresh():
        k = free[take[0] % len(free)]
        take[0] += 1
        return base_b[k].copy(), base_d[k].copy(), int(base_r[k])

    def add(tag, b, d, r):
        rows.append((b, d, r))
        tags.append(tag)

    for s in range(2):
        for subset in range(16):
            b, d, r = fresh()
            _set_bench(b, s, 0)
            for i in range(4):
                if (subset >> i) & 1:
                    _set_move(b, s, i, pp=1)
            add("pp", b, d, r)
        for _ in range(6):
            b, d, r = fresh()
            _all_slots(b, 1 - s, DISABLE, 20)
            _set_bench(b, 1 - s, 0)
            add("disable", b, d, r)
        for slot in range(1, 5):
            for own in (False, True):
                b, d, r = fresh()
                _disable(b, d, s, slot)
                if own:                                  # the side's own Haze, in the slots that are not disabled
                    for i in range(4):
                        if i + 1 != slot:
                            _set_move(b, s, i, mid=HAZE, pp=30)
                    _set_bench(b, s, 0)
                else:
                    _all_slots(b, 1 - s, HAZE, 30)
                    _set_bench(b, 1 - s, 0)
                add("haze", b, d, r)
        for slot in range(4):
            for pp in (1, 10):
                for alone in (False, True):
                    b, d, r = fresh()
                    if alone:                            # Mimic is the only move with PP: it is used at once
                        for i in range(4):
                            _set_move(b, s, i, pp=0)
                    _set_move(b, s, slot, mid=MIMIC, pp=pp)
                    _set_bench(b, s, 0)
                    add("mimic", b, d, r)
        for first in range(1, 4):
            for bench in (0, 3):
                b, d, r = fresh()
                _all_slots(b, s, TRANSFORM, 10)
                for i in range(first, 4):
                    _set_move(b, 1 - s, i, mid=0, pp=0)
                _set_bench(b, s, bench)
                add("transform", b, d, r)
        for pp in (1, 0):
            b, d, r = fresh()
            for i in range(4):
                _set_move(b, s, i, pp=pp)
            _bench_without_pp(b, s)
            add("empty", b, d, r)
    return rows, tuple(tags)


@functools.lru_cache(maxsize=None)
def _cases():
    """Every state under SEEDS choice streams, and the oracle's outcome at every cap (computed once, read-only)."""
    rows, tags = _states()
    b = np.repeat(np.stack([x[0] for x in rows]), SEEDS, axis=0)
    d = np.repeat(np.stack([x[1] for x in rows]), SEEDS, axis=0)
    r = np.repeat(np.array([x[2] for x in rows], dtype=np.uint8), SEEDS)
    p = np.zeros((len(b), 8), dtype=np.uint8)
    O.LIB.oracle_fast_prng_seed_batch(O.ptr(p), len(p), C.c_uint64(0x32C0FFEE0000))
    exp = {}
    for cap in CAPS:
        ob, od, op = b.copy(), d.copy(), p.copy()
        oout, osteps = O.rollout_batch(ob, od, r, op, max_steps=cap, threads=8)
        exp[cap] = dict(results=oout, steps=osteps, prng=op, battles=ob, durations=od)
        for a in exp[cap].values():
            a.setflags(write=False)
    for a in (b, d, r, p):
        a.setflags(write=False)
    return b, d, r, p, exp, tuple(t for t in tags for _ in range(SEEDS))


def _disabled_slot(b, s):
    return (u32(b, s * SIDE + ACTIVE + 20) >> 24) & 7


def test_the_oracle_accepts_the_cases_and_every_change_happens():
    b, d, r, p, exp, tags = _cases()
    n = len(tags)
    for cap in CAPS:
        assert ((exp[cap]["results"] & 15) != 4).all(), (cap, sorted({tags[k] for k in np.where((exp[cap]["results"] & 15) == 4)[0]}))
    seen = set()
    for k in range(n):
        imgs = [b[k]] + [exp[cap]["battles"][k] for cap in CAPS]
        for s in range(2):
            used = [int(x[s * SIDE + LAST_USED]) for x in imgs]
            dis = [_disabled_slot(x, s) for x in imgs]
            ids = [tuple(int(x[s * SIDE + ACTIVE + 24 + 2 * i]) for i in range(4)) for x in imgs]
            lead = [int(x[s * SIDE + ORDER]) for x in imgs]
            if STRUGGLE in used:
                seen.add((tags[k], "struggle"))
            seen |= {(tags[k], "disabled %d" % slot) for slot in dis[1:] if slot and dis[0] == 0}
            if any(x and not y for x, y in zip(dis, dis[1:])):
                seen.add((tags[k], "disable over"))
            if tags[k] == "mimic" and any(MIMIC in x and MIMIC not in y and lead[0] == lead[j + 1] for j, (x, y) in enumerate(zip(ids, ids[1:]))):
                seen.add((tags[k], "copied"))
            if any(_vlo(x, s) & V["TRANSFORM"] for x in imgs[1:]):
                seen.add((tags[k], "transformed"))
            back = [j for j in range(1, len(lead)) if lead[j] == lead[0] and any(l != lead[0] for l in lead[:j])]
            if back:
                seen.add((tags[k], "out and back"))
            if any(l != lead[0] for l in lead):
                seen.add((tags[k], "switched"))
    want = {("pp", "struggle"), ("disable", "disable over"), ("haze", "disable over"), ("mimic", "copied"), ("mimic", "struggle"),
            ("transform", "transformed"), ("transform", "out and back"), ("empty", "switched"), ("empty", "struggle")}
    want |= {("disable", "disabled %d" % slot) for slot in range(1, 5)}
    assert want <= seen, sorted(want - seen)


@pytest.fixture
def ctx(gpu_ctx):
    """The session's context with no lane spread; the schedule settings back to their defaults afterwards."""
    from test_gpu_move_carry import DEFAULT
    _spread(gpu_ctx, 0)
    try:
        yield gpu_ctx
    finally:
        _spread(gpu_ctx, -1)
        gpu_ctx.set_move_carry(DEFAULT)


@pytest.mark.gpu
@pytest.mark.parametrize("carry", ("off", "default"))
def test_every_cap_through_the_queue_kernel(ctx, carry):
    from test_gpu_move_carry import DEFAULT
    b, d, r, p, exp, tags = _cases()
    ctx.set_move_carry(0 if carry == "off" else DEFAULT)
    for cap in CAPS:
        got = ctx.rollout_group([(b, d, r, p)], max_steps=cap, return_state=True)[0]
        _compare(got, exp[cap], tags, ("rollout_group", carry, cap))
        assert ctx.queue_counters()[63] == 0


@pytest.mark.gpu
def test_the_cases_in_slices_of_four_turn_steps_through_k_root_step(gpu_ctx):
    """k_root_step carries a playout's registers from launch to launch: the cases as roots, a few playouts each, four turn-steps a launch."""
    from test_gpu_parity import _RootSteps, _seed_prng
    b, d, r, _, _, tags = _cases()
    b, d, r = (np.ascontiguousarray(x[::SEEDS]) for x in (b, d, r))
    reps, steps, slice_, max_steps = 4, 2, 4, 48
    lane = _seed_prng(len(b) * reps, 0xC50000000000)
    ref_lane = lane.copy()
    cnt, s2, ex = O.root_steps_reference(b, d, r, ref_lane, reps, steps, slice_, max_steps=max_steps, threads=8)
    rs = _RootSteps(gpu_ctx, b, d, r, lane, reps, slice_, max_steps=max_steps)
    try:
        k = 0
        while True:
            rec = rs.step(fresh=k < steps)
            assert rec["err"] == 0
            bad = np.where((rec["count"] != cnt[k]) | (rec["sum2"] != s2[k]))[0]
            assert bad.size == 0, (k, sorted({tags[j * SEEDS] for j in bad}))
            assert rec["turn_steps"] == ex[k], (k, rec["turn_steps"], ex[k])
            k += 1
            if k >= steps and rec["carried"] == 0:
                break
            assert k < cnt.shape[0], "playouts still in flight after the longest possible life"
        assert cnt[k:].sum() == 0 and cnt[:k].sum() == len(b) * reps * steps
        assert (rs.lane_streams() == ref_lane).all()
    finally:
        rs.close()
