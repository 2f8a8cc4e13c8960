"""The CPU oracle's damage path (oracle/gen1_engine.c: check_crit, calc_damage, adjust_damage, randomize_damage, apply_damage and
do_move's fixed-damage branch) against tests/damage_ref.py, a restatement in plain integers that shares no code with it, on the
constructed states of tests/damage_cases.py; the conditions under which those states are worth running on the GPU
(tests/test_gpu_damage_edges.py); and the reciprocal table that replaces the engine's division by the defence stat.  No GPU.

Repeats per state (damage_cases): SEEDS = 4, CHART_SEEDS = 2, NOTHING_SEEDS = 16 -- 38,320 lanes, built in about two seconds.

Psywave: both engines follow Pokemon Showdown's rule (switch OAK_PSYWAVE_SHOWDOWN at the top of gen1_engine.c): a draw from
0 .. level * 3 / 2 - 1, the action key holding the draw + 1, and a draw of 0 FAILS the move.  At level 1 that range is the one value 0,
so Psywave never does anything there; test_psywave_at_level_1 says so for the oracle, and the GPU tests compare those lanes like the
rest.  The key's byte is the draw + 1 modulo 256: above level 170 it no longer names the draw, and the HP lost picks among the two."""
import numpy as np

import damage_cases as D
import damage_ref as R
from inert_ref import ACTIVE, LAST_DAMAGE, SIDE, V, u16
from oak_amd import gamedata
from test_gpu_choice_draw import _stored, _vlo

CHART = gamedata.DATA["type_chart"]
ERROR = 4


def _key(act, s):
    """(damage roll, hit, crit, confused, Psywave byte) of player s from the 16-byte action key; the two-bit flags are 0 not rolled,
    1 false, 2 true."""
    w = int.from_bytes(bytes(act[8 * s:8 * s + 8]), "little")
    return w & 0xFF, (w >> 8) & 3, (w >> 10) & 3, (w >> 16) & 3, (w >> 48) & 0xFF


def _expected(b, act, s, lost=None):
    """What damage_ref says the mover s's move does to the plain state b, given the rolls in the key: None when it does not land
    (immune, missed, a failed Psywave), else (final damage, the quotient met the cap, critical hit).  `lost`, the HP the target lost,
    only picks among the Psywave draws that the key's byte cannot tell apart."""
    t = 1 - s
    mid = int(b[s * SIDE + ACTIVE + 24])
    name = gamedata.MOVE_NAMES[mid]
    eff, bp, mtype, acc = D.move_row(mid)
    roll, hit, crit, _, psy = _key(act, s)
    types = int(b[t * SIDE + ACTIVE + 11])
    t1, t2 = types & 15, types >> 4
    fixed = eff in ("SpecialDamage", "SuperFang")
    if not fixed and (CHART[mtype][t1] == 0 or CHART[mtype][t2] == 0):
        assert (roll, hit, crit) == (0, 0, 0), "an immune target draws nothing"
        return None
    assert hit == (0 if acc == 255 else hit) and hit != (0 if acc != 255 else 3), "255 is not rolled for, anything else is"
    if hit == 1:
        assert (roll, crit) == (0, 0)
        return None
    level = int(b[_stored(b, s, 0) + 23])
    if fixed:
        assert (roll, crit) == (0, 0)
        draw = None
        if name == "Psywave":       # the key's byte holds the draw + 1 modulo 256: past level 170 two draws share a byte
            draws = [x for x in range(max(level * 3 // 2, 1)) if (x + 1) & 255 == psy]
            assert draws and (len(draws) == 1 or level > 170), (psy, level)
            draw = lost if lost in draws else draws[0]
            if draw == 0:
                return None
        return R.fixed(name, level, u16(b, _stored(b, t, 0) + 18), u16(b, LAST_DAMAGE), draw), False, False
    assert crit in (1, 2)
    special = mtype >= 8
    if crit == 2:
        atk = u16(b, _stored(b, s, 0) + (8 if special else 2))
        def_ = u16(b, _stored(b, t, 0) + (8 if special else 4))
    else:
        atk = u16(b, s * SIDE + ACTIVE + (8 if special else 2))
        def_ = u16(b, t * SIDE + ACTIVE + (8 if special else 4))
        if _vlo(b, t) & V["LIGHTSCREEN" if special else "REFLECT"]:
            def_ *= 2
    d = R.base(level, bp, atk, def_, crit == 2, eff == "Explode")
    mine = int(b[s * SIDE + ACTIVE + 11])
    d = R.adjust(d, mtype in (mine & 15, mine >> 4), CHART[mtype][t1], CHART[mtype][t2], t1 == t2)
    if d <= 1:
        assert roll == 0, "damage of 0 or 1 is not rolled for"
    else:
        assert 217 <= roll <= 255, roll
    return R.rolled(d, roll), R.capped(level, bp, atk, def_, crit == 2, eff == "Explode"), crit == 2


def _check(b, ob, act, s):
    """Assert the oracle's turn-step ob of the plain state b against damage_ref; returns what _expected does."""
    t = 1 - s
    hp, ohp = u16(b, _stored(b, t, 0) + 18), u16(ob, _stored(ob, t, 0) + 18)
    want = _expected(b, act, s, hp - ohp)
    sub = _vlo(b, t) & V["SUBSTITUTE"]
    final = 0 if want is None else want[0]
    if final == 0:
        assert ohp == hp and D.sub_hp(ob, t) == D.sub_hp(b, t) and u16(ob, LAST_DAMAGE) == 0
    elif sub:
        left = D.sub_hp(b, t) - final
        assert ohp == hp and u16(ob, LAST_DAMAGE) == final
        assert (D.sub_hp(ob, t), bool(_vlo(ob, t) & V["SUBSTITUTE"])) == ((left, True) if left > 0 else (0, False))
    else:
        assert hp - ohp == min(final, hp) == u16(ob, LAST_DAMAGE), (hp, ohp, final, u16(ob, LAST_DAMAGE))
    return want


def test_the_oracle_computes_what_damage_ref_computes_on_the_plain_cases():
    b, d, r, p, exp, tags, mover, _ = D.cases()
    _, _, act = D.keyed()
    lanes = D.plain_subset()
    assert 3000 <= len(lanes) <= 4096 and {tags[k][0] for k in lanes} == set(D.PLAIN)
    landed = 0
    for k in lanes:
        try:
            landed += _check(b[k], exp["battles"][k], act[k], int(mover[k])) is not None
        except AssertionError as e:
            raise AssertionError((tags[k], int(mover[k])) + e.args) from None
    assert landed >= len(lanes) // 2, landed


def test_psywave_at_level_1():
    b, d, r, p, exp, tags, mover, _ = D.cases()
    _, _, act = D.keyed()
    lanes = [k for k, t in enumerate(tags) if t == ("levels", "Psywave", 1)]
    assert len(lanes) == D.SEEDS
    for k in lanes:
        s = int(mover[k])
        roll, hit, crit, _, psy = _key(act[k], s)
        assert psy == (1 if hit == 2 else 0) and roll == 0 and crit == 0
        assert u16(exp["battles"][k], _stored(b[k], 1 - s, 0) + 18) == 999 and u16(exp["battles"][k], LAST_DAMAGE) == 0
    assert any(_key(act[k], int(mover[k]))[1] == 2 for k in lanes), "Psywave never got past its accuracy roll"


def test_the_cases_reach_what_they_are_built_for():
    b, d, r, p, exp, tags, mover, state = D.cases()
    ob = exp["battles"]
    _, _, act = D.keyed()
    assert ((exp["results"] & 15) != ERROR).all() and (exp["steps"] == 1).all()
    assert {t[0] for t in tags} == set(D.FAMILIES)
    assert len(b) <= 60000
    hp = lambda img, k, s: u16(img[k], _stored(img[k], s, 0) + 18)
    operands, crits, finals, subs, users, cells, cap = set(), {}, set(), set(), set(), set(), False
    for k in (k for k, t in enumerate(tags) if t[0] in D.PLAIN):
        s, t = int(mover[k]), tags[k]
        want = _expected(b[k], act[k], s)
        if want is None:
            continue
        final, capped, crit = want
        cap |= capped and final > 0
        finals.add(min(final, 2))
        if _vlo(b[k], 1 - s) & V["SUBSTITUTE"] and final > 0:
            subs.add("breaks" if not _vlo(ob[k], 1 - s) & V["SUBSTITUTE"] else "holds")
        if t[0] == "explode":
            users.add("faints" if hp(ob, k, s) == 0 else "survives")
        if t[0] == "chart":
            cells.add(t[1:4])
        if t[0] == "stat grid":
            crits.setdefault((t[1], t[3], t[4], t[5]), set()).add(crit)
            _, kind, _, up, atk, def_ = t
            if crit:            # the party stats of the case: the grid rotated by 7 and by 4
                atk, def_ = D.GRID[(D.GRID.index(atk) + 7) % 15], D.GRID[(D.GRID.index(def_) + 4) % 15]
            else:
                def_ *= 2 if up else 1
            operands.add("both in a byte" if max(atk, def_) <= 255 else "defence wraps to 1" if def_ > 255 and (def_ // 4) & 255 == 0 else "quartered")
    assert operands == {"both in a byte", "quartered", "defence wraps to 1"}, operands
    assert len(crits) == 2 * 2 * 15 * 15 and all(v == {False, True} for v in crits.values()), sorted(c for c, v in crits.items() if v != {False, True})
    assert cap and finals == {0, 1, 2} and subs == {"breaks", "holds"} and users == {"faints", "survives"}, (cap, finals, subs, users)
    live = {(m, t1, t2) for m in range(14) for t1 in range(15) for t2 in range(15) if CHART[m][t1] * CHART[m][t2] != 0}
    assert cells == live, sorted(live - cells)
    # every fixed-damage value: what the target lost (all of its HP where that is less)
    seen = set()
    for k in (k for k, t in enumerate(tags) if t[0] == "fixed" or (t[0] == "levels" and t[1] in ("SeismicToss", "NightShade"))):
        s, t = int(mover[k]), tags[k]
        lost = hp(b, k, 1 - s) - hp(ob, k, 1 - s)
        assert lost == u16(ob[k], LAST_DAMAGE)
        level = int(b[k, _stored(b[k], s, 0) + 23])
        if t[1] == "Counter":
            want = R.fixed("Counter", level, 0, t[2], 0) if t[3] else 0
            assert lost == min(want, hp(b, k, 1 - s)), t
            seen.add(t[1:])
        elif lost:
            assert lost == min(R.fixed(t[1], level, hp(b, k, 1 - s), 0, 0), hp(b, k, 1 - s)), t
            seen.add(t[1:])
    want = ({("SuperFang", h) for h in D.FANG_HP} | {("Counter", x, c) for x in D.COUNTER_DAMAGE for c in (0, 1)} |
            {(n, t1, t2) for n in ("SonicBoom", "DragonRage") for t1, t2 in (("Ghost", "Ghost"), ("Normal", "Normal"), ("Ghost", "Normal"))} |
            {(n, lv) for n in ("SeismicToss", "NightShade") for lv in D.LEVELS})
    assert seen == want, sorted(map(str, want - seen))
    # a confused mover both hits itself and does not; the self-hit is own Attack into own Defence, behind own Reflect, without a roll
    hurt = set()
    for k in (k for k, t in enumerate(tags) if t[0] == "confusion"):
        s, (_, atk, def_, up, foe_sub) = int(mover[k]), tags[k]
        confused = _key(act[k], s)[3]
        assert confused in (1, 2)
        hurt.add(confused == 2)
        if confused == 2:
            dmg = R.base(int(b[k, _stored(b[k], s, 0) + 23]), 40, atk, def_ * (2 if up else 1), False, False)
            if foe_sub:         # the gen-1 quirk: the FOE's substitute takes it
                assert hp(ob, k, s) == 999 and D.sub_hp(ob[k], 1 - s) == max(foe_sub - dmg, 0)
            else:
                assert 999 - hp(ob, k, s) == min(dmg, 999)
    assert hurt == {False, True}
    # under Transform a critical hit works on the COPIED Pokemon's party stats on both sides
    crit_seen = 0
    for k in (k for k, t in enumerate(tags) if t[0] == "transform"):
        s, (_, atk, def_) = int(mover[k]), tags[k]
        roll, hit, crit, _, _ = _key(act[k], s)
        if crit == 2:
            crit_seen += 1
            level = int(b[k, _stored(b[k], s, 0) + 23])
            dmg = R.rolled(R.adjust(R.base(level, 70, atk, def_, True, False), True, 2, 2, True), roll)
            assert hp(b, k, 1 - s) - hp(ob, k, 1 - s) == min(dmg, 999), tags[k]
    assert crit_seen >= 64


def test_the_reciprocal_table_divides_exactly():
    """EngineR::fast_div24 (one multiply-high against rcp[d] = floor((2^32 - 1) / d) + 1, filled by stage_tables in
    oak_amd/csrc/gen1_device.hpp) is x // d for every d in 2 .. 255 and every x < 2^24: the estimate never falls as x grows, so it is
    enough that it is right just below and at every multiple of d.  calc_damage's largest dividend is 206 * 255 * 255."""
    for d in range(2, 256):
        rcp = np.uint64(0xFFFFFFFF // d + 1)
        assert int(rcp) < 1 << 32
        m = np.arange(1, (1 << 24) // d + 1, dtype=np.uint64) * np.uint64(d)
        m = m[m < 1 << 24]
        for x in (m - np.uint64(1), m):
            assert (((x * rcp) >> np.uint64(32)) == x // np.uint64(d)).all(), d
        top = 206 * 255 * 255
        assert top < 1 << 24 and (top * int(rcp)) >> 32 == top // d


def test_two_turn_steps_carry_the_first_steps_last_damage_into_counter():
    """tests/damage_cases.py's two_steps() on the oracle alone: nothing is refused, every lane plays both turn-steps, and where Counter
    is used twice into its frozen target the second one doubles what the first one dealt."""
    b, d, r, p, exp, tags = D.two_steps()
    assert ((exp["results"] & 15) != ERROR).all() and (exp["steps"] == 2).all()
    assert {t[0] for t in tags} == {"cap", "fixed", "explode"}
    twice = 0
    for k, t in enumerate(tags):
        if t[:2] != ("fixed", "Counter") or not t[3] or t[2] == 0:
            continue
        ob = exp["battles"][k]
        s = next(s for s in range(2) if int(b[k, s * SIDE + ACTIVE + 24]) == D.move("Counter"))
        o = _stored(b[k], 1 - s, 0)
        used = sum(10 - int(ob[_stored(b[k], s, 0) + 11 + 2 * i]) for i in range(4))     # PP spent: once per Counter
        if used != 2 or any(int(ob[x * SIDE + 176]) != int(b[k, x * SIDE + 176]) for x in range(2)):
            continue
        hp0 = u16(b[k], o + 18)
        first = min(R.fixed("Counter", 0, 0, t[2], 0), hp0)
        second = min(R.fixed("Counter", 0, 0, first, 0), hp0 - first)
        assert u16(ob, o + 18) == hp0 - first - second and u16(ob, LAST_DAMAGE) == second, t
        twice += 1
    assert twice >= 1, "no lane used Counter twice with both sides staying in"


def test_the_oracle_plays_every_case_on_to_the_queue_kernels_cap():
    b, d, r, p, exp, tags, _, _ = D.cases()
    far = D.queue_steps()
    assert ((far["results"] & 15) != ERROR).all() and (far["steps"] >= 1).all() and (far["steps"] <= D.QUEUE_STEPS).all()
    assert ((far["results"] & 15) != 0).sum() > len(b) // 4 and (far["steps"] == D.QUEUE_STEPS).any()
