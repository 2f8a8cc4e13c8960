"""k_rollout_queue's fast-forward of proven inert standstills (EngineR::inert_standstill) against the CPU oracle, which plays every
turn: the harvested long playouts of tests/inert_ref.py, step caps and late turns, one-condition mutations of accepted states, and
the runtime switch.  Every output byte must equal the oracle's; the control block's counters show that the skip really fired."""
import numpy as np
import pytest

import inert_ref as R
import oracle_lib as O

KEYS = ("results", "steps", "battles", "durations", "prng")
FFWD, SKIPPED = 44, 45   # OAKGPU_CTL_FAST_FORWARDED, OAKGPU_CTL_SKIPPED_STEPS (include/oakgpu.h)


def _both(gpu_ctx, b, d, p, r, cap):
    ob, od, op = b.copy(), d.copy(), p.copy()
    oout, osteps = O.rollout_batch(ob, od, r, op, max_steps=cap, threads=8)
    got = gpu_ctx.rollout(b, d, r, p, max_steps=cap, return_state=True)
    return got, dict(results=oout, steps=osteps, battles=ob, durations=od, prng=op)


def _same(got, exp, what):
    for key in KEYS:
        assert (got[key] == exp[key]).all(), (what, key, int((got[key] != exp[key]).sum() if key in ("results", "steps")
                                                             else (got[key] != exp[key]).any(axis=1).sum()))


def _accepted(b, d, res):
    return np.array([R.inert(b[i], d[i], int(res[i])) is not None for i in range(len(b))])


@pytest.mark.gpu
def test_harvested_long_playouts_equal_the_oracle_and_are_fast_forwarded(gpu_ctx):
    b, d, p, res, total, _ = R.harvest()
    gpu_ctx.set_playouts_per_lane(2)
    got, exp = _both(gpu_ctx, b, d, p, res, 700)
    c = gpu_ctx.queue_counters()
    _same(got, exp, "harvest, cap 700")
    stalemates, acc = int((total >= 999).sum()), _accepted(b, d, res)
    print("fast-forwarded %d of %d stalemates, %d turn-steps skipped of %d" % (c[FFWD], stalemates, c[SKIPPED], int(exp["steps"].sum())))
    assert c[63] == 0
    assert c[FFWD] >= 0.85 * stalemates
    # a playout that is inert from the start plays the 9 turn-steps of the standstill gate and its last one; nothing else is skipped
    assert int(np.maximum(exp["steps"][acc].astype(np.int64) - 12, 0).sum()) <= int(c[SKIPPED]) <= int(exp["steps"].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("cap,turn", [(1, None), (137, None), (700, 960), (700, 998)])
def test_step_caps_and_the_tie_at_turn_1000(gpu_ctx, cap, turn):
    b, d, p, res, _, _ = R.harvest()
    b = b.copy()
    if turn is not None:
        b[:, R.TURN], b[:, R.TURN + 1] = turn & 0xFF, turn >> 8
    gpu_ctx.set_playouts_per_lane(2)
    got, exp = _both(gpu_ctx, b, d, p, res, cap)
    c = gpu_ctx.queue_counters()
    _same(got, exp, (cap, turn))
    if turn is not None:
        assert ((exp["results"] & 15) == 3).sum() >= 200, "the fixture no longer reaches the tie at turn 1,000"
    if cap == 137 or turn == 960:     # (a launch capped at one turn-step is not a queue launch and has no counters)
        assert c[FFWD] > 100


def _mutations():
    """(name, f(b, d, k, s) -> applied?) -- one condition of the proof changed on side s of battle k."""
    def stored(b, k, s):
        return s * R.SIDE + (int(b[k, s * R.SIDE + R.ORDER]) - 1) * 24

    def status(v):
        def f(b, d, k, s):
            b[k, stored(b, k, s) + 20] = v
            return True
        return f

    def flag(bit):
        def f(b, d, k, s):
            o = s * R.SIDE + R.ACTIVE + 16 + bit // 8
            b[k, o] ^= 1 << (bit % 8)
            if b[k, o] >> (bit % 8) & 1:   # a lock goes with the move that causes it (Bide, Thrash, Solar Beam, Rage)
                b[k, s * R.SIDE + R.LAST_SEL] = {0: 117, 1: 37, 4: 76, 12: 99}.get(bit, b[k, s * R.SIDE + R.LAST_SEL])
            return True
        return f

    def disable(b, d, k, s):
        o = s * R.SIDE + R.ACTIVE
        if b[k, o + 24] == 0:
            return False
        b[k, o + 22] = (b[k, o + 22] & 0x0F) | (3 << 4)   # 3 turns left
        b[k, o + 23] = (b[k, o + 23] & 0xF8) | 1          # ... on move slot 1
        w = d[k].view(np.uint32)
        w[s] = (w[s] & ~np.uint32(15 << 21)) | np.uint32(1 << 21)
        return True

    def equal_speeds(b, d, k, s):      # beside a frozen side that still chooses freely
        x = R.side_view(b[k], d[k], s)
        if R.side_form(x, R.side_view(b[k], d[k], 1 - s), 0) is None or x["status"] != R.FRZ:
            return False
        o, f = s * R.SIDE + R.ACTIVE + 6, (1 - s) * R.SIDE + R.ACTIVE + 6
        b[k, f:f + 2] = b[k, o:o + 2]
        return True

    def foe_not_immune(b, d, k, s):
        b[k, (1 - s) * R.SIDE + R.ACTIVE + 11] = 0x00   # Normal / Normal
        return True

    def revive_bench(b, d, k, s):
        slot = int(b[k, s * R.SIDE + R.ORDER + 1])
        if slot == 0 or R.u16(b[k], s * R.SIDE + (slot - 1) * 24 + 18) != 0:
            return False
        b[k, s * R.SIDE + (slot - 1) * 24 + 18] = 1
        return True

    def poke(off_of_side, value, per_side=1):     # one byte: of side s, or of the battle (per_side = 0)
        def f(b, d, k, s):
            b[k, off_of_side + s * per_side] = value
            return True
        return f

    def attacking_duration(b, d, k, s):
        d[k].view(np.uint32)[s] |= np.uint32(1 << 25)
        return True

    names = ("BIDE", "THRASHING", "MULTIHIT", "FLINCH", "CHARGING", "BINDING", "INVULNERABLE", "CONFUSION", "MIST", "FOCUSENERGY",
             "SUBSTITUTE", "RECHARGING", "RAGE", "LEECHSEED", "TOXIC", "LIGHTSCREEN", "REFLECT")
    # (bit 17, Transform, is left to the fixture's own Ditto states: the flag without the copied Pokemon behind it is an image no
    # game reaches and no engine has to agree on)
    out = [("SLP 3", status(3)), ("PSN", status(0x08)), ("BRN", status(0x10))]
    out += [("flag " + n, flag(i)) for i, n in enumerate(names)]
    # what a paralysed side's two outcomes must agree on: last used move, its counterable bit, last damage, the attacking duration
    out += [("PAR", status(R.PAR)), ("last used 0", poke(R.LAST_USED, 0, R.SIDE)), ("counterable", poke(R.LAST_MOVES + 1, 1, 2)),
            ("last damage", poke(R.LAST_DAMAGE, 7, 0)), ("attacking duration", attacking_duration)]
    out += [("disable", disable), ("equal speeds", equal_speeds), ("foe not immune", foe_not_immune), ("bench revived", revive_bench)]
    return out


@pytest.mark.gpu
def test_one_condition_mutations_of_accepted_states(gpu_ctx):
    b, d, p, res, _, _ = R.harvest()
    acc = np.where(_accepted(b, d, res))[0]
    rows, tags = [], []
    for name, f in _mutations():
        for s in range(2):
            mb, md = b[acc].copy(), d[acc].copy()
            hit = np.array([f(mb, md, k, s) for k in range(len(acc))])
            rows.append((mb[hit], md[hit], p[acc][hit], res[acc][hit]))
            tags += [name] * int(hit.sum())
    mb, md, mp, mr = (np.concatenate([r[i] for r in rows]) for i in range(4))
    tags = np.array(tags)
    still = _accepted(mb, md, mr)
    for name, _ in _mutations():
        sel = tags == name
        print("%-16s %5d states, %5d still accepted" % (name, int(sel.sum()), int(still[sel].sum())))
        assert sel.sum() >= 8, name
        assert (~still[sel]).any() or name in ("flag MIST", "flag FOCUSENERGY", "flag SUBSTITUTE", "flag TOXIC", "flag LIGHTSCREEN",
                                               "flag REFLECT"), name   # every clause of the proof is seen failing (the unmutated states are where it holds)
    assert still.sum() >= 1000 and (~still).sum() >= 1000
    gpu_ctx.set_playouts_per_lane(2)
    got, exp = _both(gpu_ctx, mb, md, mp, mr, 700)
    bad = np.zeros(len(mb), dtype=bool)
    for key in KEYS:
        bad |= (got[key] != exp[key]) if got[key].ndim == 1 else (got[key] != exp[key]).any(axis=1)
    assert not bad.any(), sorted(set(tags[bad].tolist()))


@pytest.mark.gpu
def test_switched_off_plays_every_turn_step_to_the_same_bytes(gpu_ctx):
    b, d, p, res, _, _ = R.harvest()
    gpu_ctx.set_playouts_per_lane(2)
    fast = gpu_ctx.rollout(b, d, res, p, max_steps=700, return_state=True)
    gpu_ctx.set_standstill_skip(False)
    try:
        slow = gpu_ctx.rollout(b, d, res, p, max_steps=700, return_state=True)
        c = gpu_ctx.queue_counters()
    finally:
        gpu_ctx.set_standstill_skip(True)
    _same(slow, fast, "skip off")
    assert c[FFWD] == 0 and c[SKIPPED] == 0
