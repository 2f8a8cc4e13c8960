"""The constructed states of the damage tests (tests/test_damage_ref.py on the CPU, tests/test_gpu_damage_edges.py on the GPU) and the
oracle's one turn-step of each, computed once and handed out read-only.  CPU only.

Base states are the `free` pool of tests/test_gpu_choice_draw.py's _bases() -- both sides choose freely among four moves -- that are
_clean in the sense of tests/test_gpu_stage_scaling.py (no status, no volatile, no substitute).  In every case
  * the mover alternates between P1 and P2 and holds the move under test in all four slots;
  * the other side holds Razor Wind in all four slots: its first turn only sets the charging volatile -- no draw from battle.rng, no HP
    touched, and, unlike Splash or any other move without base power, battle.last_damage left alone -- so whatever happens to HP and to
    last_damage in the turn-step is the mover's doing whichever side is faster.  (The Counter cases freeze the other side instead: a
    charge turn clears the `counterable` byte that Counter reads, a frozen Pokemon touches nothing at all.)
  * both benches are empty, so nobody switches; accuracy and evasion stages are zero; the target has 999 of 999 HP unless the case is
    about its HP, so that a clamp to the HP left does not hide the arithmetic.
No case sets a stat to 0.

battle.rng decides every roll of a turn-step and the prng stream only which of the four identical slots is chosen, so each repeat of a
state gets a battle.rng of its own besides its own stream (oracle_fast_prng_seed_batch).  SEEDS repeats per state; the type chart's
12,600 states get CHART_SEEDS, the handful of `nothing and one` states NOTHING_SEEDS (a final damage of 2 needs the top roll, 1 in 39).
The values are the smallest round ones at which the oracle alone meets every condition of test_damage_ref.py's coverage test."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as O
from inert_ref import ACTIVE, LAST_DAMAGE, LAST_MOVES, RNG, SIDE, V
from oak_amd import gamedata
from test_gpu_choice_draw import _bases, _set_bench, _set_move, _set_vlo, _stored, _vlo
from test_gpu_stage_scaling import _clean

SEEDS, CHART_SEEDS, NOTHING_SEEDS = 4, 2, 16
GRID = (1, 2, 3, 4, 5, 255, 256, 257, 259, 260, 511, 512, 513, 998, 999)
LEVELS = (1, 2, 3, 5, 50, 99, 100, 101, 127, 128, 170, 171, 200, 255)
LEVEL_MOVES = ("Pound", "Slash", "HyperBeam", "SelfDestruct", "Explosion", "SeismicToss", "NightShade", "Psywave")
FANG_HP = (1, 2, 3, 4, 701, 999)
COUNTER_DAMAGE = (0, 1, 2, 32767, 32768, 65535)
SELF_STATS = (1, 255, 256, 999)
EXPLODE_DEF = (1, 2, 3, 255, 256, 511, 512, 999)
PLAIN = ("stat grid", "levels", "cap", "chart", "nothing and one", "explode")
FAMILIES = PLAIN + ("fixed", "confusion", "transform")
FRZ = 0x20
CHART = gamedata.DATA["type_chart"]
TYPES = {n: i for i, n in enumerate(gamedata.TYPE_NAMES)}
# one move per type that some damaging, non-fixed move carries (Dragon has Dragon Rage alone): none that poisons or burns, whose residual
# damage would fall on the target within the turn-step, and none that hits more than once
CHART_MOVES = ("Pound", "LowKick", "WingAttack", "Acid", "Earthquake", "RockSlide", "LeechLife", "Lick", "FireSpin", "WaterGun", "VineWhip",
               "ThunderShock", "Psychic", "AuroraBeam")     # (nor one that confuses: the target would hit itself)


def move(name):
    return gamedata.MOVE_NAMES.index(name)


def move_row(mid):
    """(effect name, base power, type, accuracy byte) of a move."""
    eff, bp, mtype, acc = gamedata.MOVES[mid - 1][:4]
    return gamedata.EFFECT_NAMES[eff], bp, mtype, acc


def put16(b, o, v):
    b[o], b[o + 1] = v & 0xFF, v >> 8


def stat_offsets(b, s, idx):
    """(active, stored) offset of stat idx (0 hp 1 atk 2 def 3 spe 4 spc) of side s."""
    return s * SIDE + ACTIVE + 2 * idx, _stored(b, s, 0) + 2 * idx


def set_stat(b, s, idx, active, stored=None):
    a, st = stat_offsets(b, s, idx)
    put16(b, a, active)
    put16(b, st, active if stored is None else stored)


def set_hp(b, s, hp, top=None):
    """The active Pokemon of side s at `hp` of max(top, hp) HP."""
    top = max(hp, top or 0)
    set_stat(b, s, 0, top)
    put16(b, _stored(b, s, 0) + 18, hp)


def set_types(b, s, t1, t2):
    b[s * SIDE + ACTIVE + 11] = t1 | t2 << 4


def set_level(b, s, level):
    b[_stored(b, s, 0) + 23] = level


def set_sub(b, s, hp):
    _set_vlo(b, s, _vlo(b, s) | V["SUBSTITUTE"])
    b[s * SIDE + ACTIVE + 21] = hp          # bits 40-47 of the volatiles


def sub_hp(b, s):
    return int(b[s * SIDE + ACTIVE + 21])


def other_type(t):
    """A type that is not t (for a mover without the same-type bonus)."""
    return (t + 1) % 15


@functools.lru_cache(maxsize=None)
def pre_chart_stats(bp, want):
    """(level, atk, def) at which a non-critical hit of base power bp has base damage `want`."""
    for level in (100, 50, 20, 10):
        for atk in range(1, 256):
            for def_ in (100, 60, 200, 255, 30, 10):
                if ((level * 2 // 5 + 2) * bp * atk // def_) // 50 + 2 == want:
                    return level, atk, def_
    raise AssertionError((bp, want))


@functools.lru_cache(maxsize=None)
def states():
    """(rows of (battle, durations, result), per row: the tag, the mover, the repeats)."""
    base_b, base_d, base_r, free, _ = _bases()
    pool = [k for k in free if _clean(base_b, k)]
    assert len(pool) >= 16, len(pool)
    spe = lambda k, s: gamedata.SPECIES[int(base_b[k, _stored(base_b[k], s, 0) + 21]) - 1][3]
    fast = [[k for k in pool if spe(k, s) >= 64] for s in range(2)]
    assert min(len(fast[0]), len(fast[1])) >= 8, (len(fast[0]), len(fast[1]))
    rows, tags, movers, reps, take = [], [], [], [], [0]
    razor_wind = move("RazorWind")

    def fresh(mid, quick=False):
        """A base state with the next mover: the move under test on it, Razor Wind on the other side, nobody on either bench."""
        s = take[0] % 2
        src = fast[s] if quick else pool
        k = src[(take[0] // 2) % len(src)]
        take[0] += 1
        b, d, r = base_b[k].copy(), base_d[k].copy(), int(base_r[k])
        for side, m in ((s, mid), (1 - s, razor_wind)):
            for i in range(4):
                _set_move(b, side, i, mid=m, pp=10)
            _set_bench(b, side, 0)
            b[side * SIDE + ACTIVE + 14] = 0     # accuracy and evasion stages
        set_hp(b, 1 - s, 999)
        return b, d, r, s

    def add(tag, b, d, r, s, n=SEEDS):
        rows.append((b, d, r))
        tags.append(tag)
        movers.append(s)
        reps.append(n)

    # ---- stat grid
    for kind, plain, high in (("physical", "Pound", "Slash"), ("special", "WaterGun", "RazorLeaf")):
        own, foes, screen = (1, 2, V["REFLECT"]) if kind == "physical" else (4, 4, V["LIGHTSCREEN"])
        for run, name in (("plain", plain), ("high", high), ("focus", high)):
            assert move_row(move(name))[0] == ("None" if run == "plain" else "HighCritical") and (move_row(move(name))[2] >= 8) == (kind == "special")
            for up in (0, 1):
                for i, atk in enumerate(GRID):
                    for j, def_ in enumerate(GRID):
                        b, d, r, s = fresh(move(name), quick=True)
                        set_stat(b, s, own, atk, GRID[(i + 7) % 15])
                        set_stat(b, 1 - s, foes, def_, GRID[(j + 4) % 15])
                        set_types(b, 1 - s, TYPES["Normal"], TYPES["Normal"])
                        if up:
                            _set_vlo(b, 1 - s, _vlo(b, 1 - s) | screen)
                        if run == "focus":
                            _set_vlo(b, s, _vlo(b, s) | V["FOCUSENERGY"])
                        add(("stat grid", kind, run, up, atk, def_), b, d, r, s)
    # ---- levels
    for level in LEVELS:
        for name in LEVEL_MOVES:
            b, d, r, s = fresh(move(name))
            set_level(b, s, level)
            add(("levels", name, level), b, d, r, s)
    # ---- cap and clamp: a quotient past 997, the same-type bonus and 4x on top, into full HP, 1 HP and a substitute at 1 and at full HP
    for name, target in (("Earthquake", ("Fire", "Rock")), ("Surf", ("Rock", "Ground")), ("HyperBeam", ("Normal", "Normal"))):
        mtype = move_row(move(name))[2]
        for atk, def_ in ((255, 1), (999, 40), (512, 4)):
            for variant in ("full", "1 hp", "sub 1", "sub full"):
                b, d, r, s = fresh(move(name))
                set_stat(b, s, 4 if mtype >= 8 else 1, atk)
                set_stat(b, 1 - s, 4 if mtype >= 8 else 2, def_)
                set_types(b, s, mtype, mtype)
                set_types(b, 1 - s, TYPES[target[0]], TYPES[target[1]])
                if variant == "1 hp":
                    set_hp(b, 1 - s, 1, 999)
                elif variant != "full":
                    set_sub(b, 1 - s, 1 if variant == "sub 1" else 999 // 4 + 1)
                add(("cap", name, atk, def_, variant), b, d, r, s)
    # ---- type chart
    for name in CHART_MOVES:
        mid = move(name)
        eff, bp, mtype, _ = move_row(mid)
        assert mtype == CHART_MOVES.index(name) and bp > 0 and eff not in ("SpecialDamage", "SuperFang", "OHKO")
        for t1 in range(15):
            for t2 in range(15):
                for stab in (0, 1):
                    for want in ((7, 5, 3)[(t1 + t2) % 3], 151):
                        level, atk, def_ = pre_chart_stats(bp, want)
                        b, d, r, s = fresh(mid)
                        set_level(b, s, level)
                        set_stat(b, s, 4 if mtype >= 8 else 1, atk)
                        set_stat(b, 1 - s, 4 if mtype >= 8 else 2, def_)
                        mine = mtype if stab else other_type(mtype)
                        set_types(b, s, mine, mine)
                        set_types(b, 1 - s, t1, t2)
                        add(("chart", mtype, t1, t2, stab, want), b, d, r, s, CHART_SEEDS)
    assert {gamedata.MOVES[m - 1][2] for m in range(1, 165) if move_row(m)[1] > 0 and move_row(m)[0] not in ("SpecialDamage", "SuperFang", "OHKO")
            and m != move("Counter")} == set(range(14))
    # ---- nothing and one: base damage 2 under 1x, 1/2x and 1/4x (Normal is halved by Rock alone, so the Normal moves stop at 1/2x)
    for name in ("Pound", "Tackle", "Bind", "Wrap", "WaterGun", "Bubble", "Clamp", "VineWhip"):
        mid = move(name)
        _, bp, mtype, _ = move_row(mid)
        assert 15 <= bp <= 40
        halves = [t for t in range(15) if CHART[mtype][t] == 1]
        neutral = next(t for t in range(15) if CHART[mtype][t] == 2)
        targets = [(neutral, neutral), (halves[0], neutral)] + ([(halves[0], halves[1])] if len(halves) > 1 else [])
        for t1, t2 in targets:
            for stab in (0, 1):
                b, d, r, s = fresh(mid)
                set_level(b, s, 1)
                set_stat(b, s, 4 if mtype >= 8 else 1, 1)
                set_stat(b, 1 - s, 4 if mtype >= 8 else 2, 255)
                mine = mtype if stab else other_type(mtype)
                set_types(b, s, mine, mine)
                set_types(b, 1 - s, t1, t2)
                add(("nothing and one", name, CHART[mtype][t1] * CHART[mtype][t2], stab), b, d, r, s, NOTHING_SEEDS)
    # ---- explode: into a bare target, a substitute that breaks (1 HP) and one that holds (level 1, Attack 4: at most 44 into 255)
    for name in ("SelfDestruct", "Explosion"):
        for def_ in EXPLODE_DEF:
            for up in (0, 1):
                for variant in ("bare", "sub breaks", "sub holds"):
                    b, d, r, s = fresh(move(name))
                    set_stat(b, 1 - s, 2, def_)
                    set_types(b, 1 - s, TYPES["Normal"], TYPES["Normal"])
                    if up:
                        _set_vlo(b, 1 - s, _vlo(b, 1 - s) | V["REFLECT"])
                    if variant == "sub breaks":
                        set_sub(b, 1 - s, 1)
                    elif variant == "sub holds":
                        set_level(b, s, 1)
                        set_stat(b, s, 1, 4)
                        set_sub(b, 1 - s, 255)
                    add(("explode", name, def_, up, variant), b, d, r, s)
    # ---- fixed damage
    for hp in FANG_HP:
        for _ in range(2):
            b, d, r, s = fresh(move("SuperFang"))
            set_hp(b, 1 - s, hp, 999)
            add(("fixed", "SuperFang", hp), b, d, r, s)
    for last in COUNTER_DAMAGE:
        for counterable in (0, 1):
            for _ in range(2):
                b, d, r, s = fresh(move("Counter"))
                put16(b, LAST_DAMAGE, last)
                b[LAST_MOVES + 2 * (1 - s) + 1] = counterable
                b[_stored(b, 1 - s, 0) + 20] = FRZ
                add(("fixed", "Counter", last, counterable), b, d, r, s)
    for name in ("SonicBoom", "DragonRage"):
        for t1, t2 in (("Ghost", "Ghost"), ("Normal", "Normal"), ("Ghost", "Normal")):
            for _ in range(2):
                b, d, r, s = fresh(move(name))
                set_types(b, 1 - s, TYPES[t1], TYPES[t2])
                add(("fixed", name, t1, t2), b, d, r, s)
    # ---- confusion self-hit: own Attack into own Defence behind own Reflect, absorbed by the FOE's substitute when it has one
    for atk in SELF_STATS:
        for def_ in SELF_STATS:
            for up in (0, 1):
                for foe_sub in (0, 10, 200):
                    b, d, r, s = fresh(move("Pound"))
                    set_stat(b, s, 1, atk)
                    set_stat(b, s, 2, def_)
                    set_hp(b, s, 999)
                    _set_vlo(b, s, _vlo(b, s) | V["CONFUSION"] | 3 << 18 | (V["REFLECT"] if up else 0))    # three turns left
                    w = d.view(np.uint32)
                    w[s] = (w[s] & ~np.uint32(7 << 18)) | np.uint32(1 << 18)
                    if foe_sub:
                        set_sub(b, 1 - s, foe_sub)
                    add(("confusion", atk, def_, up, foe_sub), b, d, r, s)
    # ---- transform: the mover is a copy of the foe's active Pokemon; a critical hit reads the COPIED Pokemon's party stats for both sides
    for atk in SELF_STATS:
        for def_ in SELF_STATS:
            for _ in range(2):
                b, d, r, s = fresh(move("Slash"), quick=True)
                f = 1 - s
                put16(b, _stored(b, f, 0) + 2, atk)
                put16(b, _stored(b, f, 0) + 4, def_)
                set_types(b, f, TYPES["Normal"], TYPES["Normal"])
                so, fo = s * SIDE + ACTIVE, f * SIDE + ACTIVE
                b[so:so + 16] = b[fo:fo + 16]        # stats, species, types, stages
                _set_vlo(b, s, _vlo(b, s) | V["TRANSFORM"])
                b[so + 22] = (int(b[so + 22]) & 0xF0) | (f << 3 | int(b[f * SIDE + 176]))   # bits 48-51: side << 3 | party id
                for i in range(4):
                    b[so + 24 + 2 * i], b[so + 25 + 2 * i] = move("Slash"), 5
                add(("transform", atk, def_), b, d, r, s)
    return tuple(rows), tuple(tags), tuple(movers), tuple(reps)


@functools.lru_cache(maxsize=None)
def cases():
    """Every lane: (battles, durations, results, prng, the oracle's turn-step of each, tag, mover and state index per lane)."""
    rows, tags, movers, reps = states()
    n = np.array(reps)
    b = np.repeat(np.stack([x[0] for x in rows]), n, axis=0)
    d = np.repeat(np.stack([x[1] for x in rows]), n, axis=0)
    r = np.repeat(np.array([x[2] for x in rows], dtype=np.uint8), n)
    state = np.repeat(np.arange(len(rows)), n)
    b[:, RNG:RNG + 8] = np.random.default_rng(0x3D4A).integers(0, 256, (len(b), 8), dtype=np.uint8)
    p = np.zeros((len(b), 8), dtype=np.uint8)
    O.LIB.oracle_fast_prng_seed_batch(O.ptr(p), len(p), C.c_uint64(0x3DC0FFEE0000))
    ob, od, op = b.copy(), d.copy(), p.copy()
    oout, osteps = O.rollout_batch(ob, od, r, op, max_steps=1, threads=8)
    exp = dict(results=oout, steps=osteps, prng=op, battles=ob, durations=od)
    mover = np.repeat(np.array(movers), n)
    for a in (b, d, r, p, mover, state) + tuple(exp.values()):
        a.setflags(write=False)
    return b, d, r, p, exp, tuple(tags[k] for k in state), mover, state


@functools.lru_cache(maxsize=None)
def keyed():
    """The same turn-step of every lane once more through oracle_update, which also gives the 16-byte chance-action key: (P1's choice,
    P2's choice, actions), the choices drawn as the rollout draws them.  It must reproduce cases()'s expectation byte for byte."""
    b, d, r, p, exp, tags, _, _ = cases()
    c1, c2, act = np.zeros(len(b), np.uint8), np.zeros(len(b), np.uint8), np.zeros((len(b), 16), np.uint8)
    opt = O.Options()
    for k in range(len(b)):
        seed = O.LIB.oracle_fast_prng_uniform_64(O.ptr(p[k].copy()))
        ch1, ch2 = O.choices(b[k], 0, (int(r[k]) >> 4) & 3), O.choices(b[k], 1, (int(r[k]) >> 6) & 3)
        c1[k], c2[k] = ch1[seed % len(ch1)], ch2[(seed >> 32) % len(ch2)]
        img = b[k].copy()
        opt.set(d[k])
        res = O.update(img, int(c1[k]), int(c2[k]), opt)
        assert res == exp["results"][k] and (img == exp["battles"][k]).all() and (opt.durations == exp["durations"][k]).all(), tags[k]
        act[k] = opt.actions
    for a in (c1, c2, act):
        a.setflags(write=False)
    return c1, c2, act


@functools.lru_cache(maxsize=None)
def plain_subset():
    """At most 4,096 lanes of the plain families, the first repeat of a state each: every state of the small families, a fixed random
    draw of the stat grid's and the type chart's."""
    _, tags, _, reps = states()
    first = np.concatenate(([0], np.cumsum(reps)[:-1]))
    rng = np.random.default_rng(0x3D4B)
    pick = []
    for fam, most in (("stat grid", 1400), ("levels", None), ("cap", None), ("chart", 2200), ("nothing and one", None), ("explode", None)):
        idx = np.array([k for k, t in enumerate(tags) if t[0] == fam])
        if most is not None and len(idx) > most:
            idx = np.sort(rng.choice(idx, most, replace=False))
        pick.append(first[idx])
    out = np.concatenate(pick)
    assert len(out) <= 4096, len(out)
    out.setflags(write=False)
    return out


QUEUE_STEPS = 17      # the smallest cap at which a group launch runs the queue kernel (and with it the lean instantiation)


@functools.lru_cache(maxsize=None)
def queue_steps():
    """The oracle's QUEUE_STEPS turn-steps of every lane of cases(): with nobody on either bench most games are over by then."""
    b, d, r, p, _, _, _, _ = cases()
    ob, od, op = b.copy(), d.copy(), p.copy()
    oout, osteps = O.rollout_batch(ob, od, r, op, max_steps=QUEUE_STEPS, threads=8)
    exp = dict(results=oout, steps=osteps, prng=op, battles=ob, durations=od)
    for a in exp.values():
        a.setflags(write=False)
    return exp


@functools.lru_cache(maxsize=None)
def two_steps():
    """The cap, fixed and explode lanes with ONE live bench Pokemon on either side, and the oracle's two turn-steps of each: the second
    one follows a faint (a switch request), a broken substitute, a Hyper Beam (the recharge), and reads the last_damage the first one
    left -- Counter in particular, whose frozen target keeps its `counterable` byte.  (A side now also has the switch to choose, one
    choice in five.)  Returns (battles, durations, results, prng, expectation, tags)."""
    b, d, r, p, _, tags, _, _ = cases()
    lanes = np.array([k for k, t in enumerate(tags) if t[0] in ("cap", "fixed", "explode")])
    b, d, r, p = b[lanes].copy(), d[lanes].copy(), r[lanes].copy(), p[lanes].copy()
    for k in range(len(b)):
        for s in range(2):
            _set_bench(b[k], s, 1)
    ob, od, op = b.copy(), d.copy(), p.copy()
    oout, osteps = O.rollout_batch(ob, od, r, op, max_steps=2, threads=8)
    exp = dict(results=oout, steps=osteps, prng=op, battles=ob, durations=od)
    for a in (b, d, r, p) + tuple(exp.values()):
        a.setflags(write=False)
    return b, d, r, p, exp, tuple(tags[k] for k in lanes)


ROLLS = (1, 2, 3, 20, 39)      # the clamps oakgpu_tree_step_dev takes (include/oakgpu.h); 39 is no clamp


def roll_byte(rolls, seed):
    """tests/test_gpu_move_coverage.py's: the override byte of a clamp to `rolls` damage rolls, from a byte of battle.rng."""
    return 236 if rolls == 1 else 217 + (38 // (rolls - 1)) * (seed % rolls)


@functools.lru_cache(maxsize=None)
def roll_cases(count=256):
    """`count` lanes of the plain subset and, per clamp of ROLLS, the oracle's turn-step under that clamp's override bytes:
    (lanes, {rolls: (battles, durations, results, actions, P1's next choices, P2's)})."""
    b, d, r, _, _, _, _, _ = cases()
    c1, c2, _ = keyed()
    sub = plain_subset()
    lanes = sub[np.linspace(0, len(sub) - 1, count).astype(np.int64)]
    out = {}
    opt = O.Options()
    for rolls in ROLLS:
        ob, od = b[lanes].copy(), d[lanes].copy()
        ores, oact = np.zeros(count, np.uint8), np.zeros((count, 16), np.uint8)
        nxt = [[], []]
        for i, k in enumerate(lanes):
            over = None
            if rolls != 39:
                over = np.zeros(16, np.uint8)
                over[0], over[8] = roll_byte(rolls, int(b[k, RNG + 6])), roll_byte(rolls, int(b[k, RNG + 7]))
            opt.set(d[k], over)
            ores[i] = O.update(ob[i], int(c1[k]), int(c2[k]), opt)
            od[i], oact[i] = opt.durations, opt.actions
            for pl in range(2):
                nxt[pl].append(O.choices(ob[i], pl, (int(ores[i]) >> (4 + 2 * pl)) & 3) if (int(ores[i]) & 15) == 0 else None)
        out[rolls] = (ob, od, ores, oact, tuple(nxt[0]), tuple(nxt[1]))
    return lanes, out
