"""The constructed states of the turn-bookkeeping tests (tests/test_clock_ref.py on the CPU, tests/test_gpu_clock_edges.py on the GPU)
and the oracle's turn-steps of each, computed once and handed out read-only.  CPU only.

Base states are the clean `free` pool of tests/damage_cases.py.  In every case the SUBJECT (P1 and P2 in turn, acting first and acting
second in turn: its active Speed is 200 against 100, or 100 against 200) holds the move under test in all four slots, the other side
holds Splash in all four -- no draw, no damage, last_damage 0 -- and both benches are empty unless the case is about a switch or a
faint with somebody left, so the choice stream cannot change what is played.  Every lane has a battle.rng of its own.

Families (FAMILIES): residual (poison, burn, Toxic, Leech Seed on the max HP x status x seed x HP x foe HP grid, and the extras: a
sleeping, a frozen, a switching, a foe-fainting and a Transformed holder), heal (Recover, Soft-Boiled, Rest), substitute, and the clocks
sleep, confusion, disable, thrash, binding (a running one each, and `starts`, the first turn of each), flinch / recharge, and a full
paralysis or a confusion self-hit over each lock.  A tag is (family, kind, subject, acts first, parameters ...); cases() also gives
the parameters by name.

19,284 states, 23,832 lanes: SEEDS = 6 where a draw decides, SWITCH_SEEDS = 16 where the choice stream has to pick a switch (one
choice in five), START_SEEDS = 96 where a clock's first length is drawn (a Disable that has to hit and then draw an 8), one lane
otherwise -- the smallest round values at which the oracle alone meets every condition of tests/test_clock_ref.py.  Built, stepped
and keyed in about three seconds."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as O
from damage_cases import QUEUE_STEPS, TYPES, move, put16, set_hp, set_stat, set_sub, set_types, sub_hp  # noqa: F401
from inert_ref import ACTIVE, LAST_DAMAGE, LAST_MOVES, LAST_SEL, RNG, SIDE, V
from test_gpu_choice_draw import _bases, _set_bench, _set_move, _set_vlo, _stored, _vlo
from test_gpu_stage_scaling import _clean

SEEDS, SWITCH_SEEDS, START_SEEDS = 6, 16, 96
PSN, BRN, FRZ, PAR, EXT, TOX = 0x08, 0x10, 0x20, 0x40, 0x80, 0x88
FAMILIES = ("residual", "heal", "substitute", "sleep", "confusion", "disable", "thrash", "binding", "starts", "flinch", "locks")
MAX_HP = (1, 15, 16, 17, 31, 32, 33, 255, 256, 703, 999)
TOXIC_CTR = (0, 1, 14, 15, 16, 30, 31)
STATUSES = (("psn", None), ("brn", None)) + tuple(("tox", c) for c in TOXIC_CTR) + ((None, None),)     # (None: Leech Seed alone)
HEAL_MAX = (1, 2, 3, 255, 256, 257, 511, 512, 703, 999)
HEAL_MOVES = ("Recover", "SoftBoiled", "Rest")
SUB_MAX = (1, 2, 3, 4, 5, 7, 8, 999)
BIND_DAMAGE = (0, 1, 700, 65535)
DURS = (1, 2, 6, 7)             # duration values of the thrash and binding cases: the first ones and the last ones of the 3-bit field
# the locks a full paralysis or a confusion self-hit ends: name -> (volatile bits, selected move, attack counter, the durations field)
LOCKS = {"thrash": (V["THRASHING"], "Thrash", 3, 25), "charging": (V["CHARGING"], "SolarBeam", 0, None), "bide": (V["BIDE"], "Bide", 2, 25),
         "binding": (V["BINDING"], "Wrap", 3, 28), "invulnerable": (V["CHARGING"] | V["INVULNERABLE"], "Fly", 0, None),
         "multihit": (V["MULTIHIT"], "Splash", 0, None)}
D_SLEEP0, D_CONFUSION, D_DISABLE, D_ATTACKING, D_BINDING = (0, 3), (18, 3), (21, 4), (25, 3), (28, 3)     # (shift, bits) in a side's word


def dget(d, s, field):
    return (int(d.view(np.uint32)[s]) >> field[0]) & ((1 << field[1]) - 1)


def dset(d, s, field, x):
    w = d.view(np.uint32)
    mask = ((1 << field[1]) - 1) << field[0]
    w[s] = (int(w[s]) & ~mask) | (x << field[0] & mask)


def status_at(b, s, pos=0):
    return int(b[_stored(b, s, pos) + 20])


def set_status(b, s, v, pos=0):
    b[_stored(b, s, pos) + 20] = v


# the counters inside the volatiles: confusion (bits 18-20) and attacks (21-23) in the lower word, disable and toxic in the upper
def conf_left(b, s):
    return (_vlo(b, s) >> 18) & 7


def attacks(b, s):
    return (_vlo(b, s) >> 21) & 7


def set_counter(b, s, shift, x):
    _set_vlo(b, s, (_vlo(b, s) & ~(7 << shift)) | x << shift)


def disable_of(b, s):
    """(turns left, slot)"""
    o = s * SIDE + ACTIVE
    return int(b[o + 22]) >> 4, int(b[o + 23]) & 7


def set_disable(b, s, left, slot):
    o = s * SIDE + ACTIVE
    b[o + 22] = (int(b[o + 22]) & 0x0F) | left << 4
    b[o + 23] = (int(b[o + 23]) & 0xF8) | slot


def toxic_ctr(b, s):
    return int(b[s * SIDE + ACTIVE + 23]) >> 3


def set_toxic(b, s, ctr):
    set_status(b, s, TOX)
    _set_vlo(b, s, _vlo(b, s) | V["TOXIC"])
    o = s * SIDE + ACTIVE + 23
    b[o] = (int(b[o]) & 7) | ctr << 3


def pp_sum(b, s):
    return sum(int(b[s * SIDE + ACTIVE + 25 + 2 * i]) for i in range(4))


def hp_of(b, s, pos=0):
    o = _stored(b, s, pos) + 18
    return int(b[o]) | int(b[o + 1]) << 8


def max_hp_of(b, s, pos=0):
    o = _stored(b, s, pos)
    return int(b[o]) | int(b[o + 1]) << 8


def residual_hp(max_hp, tick):
    return sorted({h for h in (1, tick - 1, tick, tick + 1, max_hp) if 1 <= h <= max_hp})


@functools.lru_cache(maxsize=None)
def states():
    """(rows of (battle, durations, result), per row: the tag, the spec, the repeats)."""
    base_b, base_d, base_r, free, _ = _bases()
    pool = [k for k in free if _clean(base_b, k)]
    assert len(pool) >= 16, len(pool)
    rows, tags, specs, reps, take = [], [], [], [], [0]

    def fresh(s, first, name, foe="Splash"):
        k = pool[take[0] % len(pool)]
        take[0] += 1
        b, d, r = base_b[k].copy(), base_d[k].copy(), int(base_r[k])
        for side, m in ((s, move(name)), (1 - s, move(foe))):
            for i in range(4):
                _set_move(b, side, i, mid=m, pp=10)
            _set_bench(b, side, 0)
            b[side * SIDE + ACTIVE + 14] = 0     # accuracy and evasion stages
            set_stat(b, side, 3, 200 if (side == s) == bool(first) else 100)
            w = d.view(np.uint32)
            w[side] = int(w[side]) & 0x3FFF8         # no duration but the bench's sleeps
        put16(b, LAST_DAMAGE, 0)
        return b, d, r

    def add(family, kind, s, first, b, d, r, n=1, **spec):
        rows.append((b, d, r))
        tags.append((family, kind, s, first) + tuple(spec.values()))
        specs.append(dict(spec, family=family, kind=kind, s=s, first=first))
        reps.append(n)

    def afflict(b, s, status, ctr, seeded):
        if status == "tox":
            set_toxic(b, s, ctr)
        elif status:
            set_status(b, s, PSN if status == "psn" else BRN)
        if seeded:
            _set_vlo(b, s, _vlo(b, s) | V["LEECHSEED"])

    each = [(s, first) for s in range(2) for first in (1, 0)]
    # ---- residual: the grid
    for max_hp in MAX_HP:
        tick = max(1, max_hp // 16)
        for status, ctr in STATUSES:
            for seeded in ((1,) if status is None else (0, 1)):
                # the largest tick of the turn-step: the one the seed takes, where the cap on the foe's side lies
                last = tick * (((ctr + 1 + seeded) & 31) if status == "tox" else 1)
                for hp in residual_hp(max_hp, tick):
                    for foe_hp in sorted({h for h in (0, 1, 999 - last, 999 - last + 1, 999) if 0 <= h <= 999}):
                        for s, first in each:
                            b, d, r = fresh(s, first, "Splash")
                            set_hp(b, s, hp, max_hp)
                            afflict(b, s, status, ctr, seeded)
                            set_hp(b, 1 - s, foe_hp, 999)
                            if foe_hp == 0:
                                _set_bench(b, 1 - s, 1)
                            add("residual", "grid", s, first, b, d, r, max_hp=max_hp, status=status, ctr=ctr, seeded=seeded, hp=hp, foe_hp=foe_hp)
    # ---- residual: the extras
    for s, first in each:
        for kind, status_byte in (("asleep", 3), ("frozen", FRZ)):       # the residual still runs
            for max_hp, hp in ((15, 1), (160, 10), (160, 11), (703, 703)):
                b, d, r = fresh(s, first, "Splash")
                set_hp(b, s, hp, max_hp)
                set_status(b, s, status_byte)
                if kind == "asleep":
                    dset(d, s, D_SLEEP0, 1)
                _set_vlo(b, s, _vlo(b, s) | V["LEECHSEED"])
                set_hp(b, 1 - s, 500, 999)
                add("residual", kind, s, first, b, d, r, max_hp=max_hp, hp=hp)
        for status, ctr in (("psn", None), ("tox", 3)):
            # a holder that may switch (one live bench Pokemon: one choice in five): no residual for the one that left
            b, d, r = fresh(s, first, "Splash")
            set_hp(b, s, 100, 160)
            afflict(b, s, status, ctr, 1)
            _set_bench(b, s, 1)
            set_hp(b, 1 - s, 500, 999)
            add("residual", "switch", s, first, b, d, r, SWITCH_SEEDS, status=status, ctr=ctr)
            # a holder whose move faints the foe: no residual (Swift never misses; the foe is Normal and has 1 HP)
            b, d, r = fresh(s, first, "Swift")
            set_hp(b, s, 100, 160)
            afflict(b, s, status, ctr, 1)
            set_hp(b, 1 - s, 1, 999)
            set_types(b, 1 - s, TYPES["Normal"], TYPES["Normal"])
            add("residual", "faints the foe", s, first, b, d, r, status=status, ctr=ctr)
            # a Transformed holder: the max HP is the party entry's own (160), not the copy's (999)
            for hp in (9, 10, 11, 160):
                b, d, r = fresh(s, first, "Splash")
                set_hp(b, s, hp, 160)
                put16(b, s * SIDE + ACTIVE, 999)
                afflict(b, s, status, ctr, 1)
                _set_vlo(b, s, _vlo(b, s) | V["TRANSFORM"])
                o = s * SIDE + ACTIVE + 22
                b[o] = (int(b[o]) & 0xF0) | ((1 - s) << 3 | int(b[(1 - s) * SIDE + 176]))
                set_hp(b, 1 - s, 500, 999)
                add("residual", "transformed", s, first, b, d, r, status=status, ctr=ctr, hp=hp)
    # ---- heal
    for name in HEAL_MOVES:
        for max_hp in HEAL_MAX:
            half = max_hp // 2
            for lost in sorted({x for x in (0, 1, half - 1, half, half + 1, 254, 255, 256, 510, 511, 512, 767) if 0 <= x < max_hp}):
                for s, first in each:
                    b, d, r = fresh(s, first, name)
                    set_hp(b, s, max_hp - lost, max_hp)
                    dset(d, s, D_SLEEP0, 5)      # a stale value: Rest resets it
                    add("heal", name, s, first, b, d, r, max_hp=max_hp, lost=lost, status=None)
    for status in ("psn", "tox", "brn", "par"):
        for lost in (0, 255, 300):
            for s, first in each:
                b, d, r = fresh(s, first, "Rest")
                set_hp(b, s, 703 - lost, 703)
                if status == "par":
                    set_status(b, s, PAR)
                else:
                    afflict(b, s, status, 5, 0)
                set_stat(b, s, 1, 77, 154)                           # the halved Attack and the quartered Speed stay as they are
                set_stat(b, s, 3, 201 if first else 25, 100)
                set_stat(b, 1 - s, 3, 100)
                dset(d, s, D_SLEEP0, 5)
                add("heal", "Rest", s, first, b, d, r, SEEDS if status == "par" else 1, max_hp=703, lost=lost, status=status)
    # ---- substitute
    for max_hp in SUB_MAX:
        cost = max_hp // 4
        for hp in sorted({h for h in (cost - 1, cost, cost + 1, max_hp) if 1 <= h <= max_hp}):
            for has_one in (0, 1):
                for bench in ((0, 1) if hp == cost and not has_one else (0,)):
                    for s, first in each:
                        b, d, r = fresh(s, first, "Substitute")
                        set_hp(b, s, hp, max_hp)
                        if has_one:
                            set_sub(b, s, 7)
                        _set_bench(b, s, bench)
                        add("substitute", "bench" if bench else "alone", s, first, b, d, r, SWITCH_SEEDS if bench else 1,
                            max_hp=max_hp, hp=hp, has_one=has_one)
    # ---- sleep: the byte 1 .. 7 with every duration value it can carry, 1 .. 7 extended (3 .. 7: compared only)
    for s, first in each:
        for ctr in range(1, 8):
            for dur in range(1, 9 - ctr):
                b, d, r = fresh(s, first, "Splash")
                set_status(b, s, ctr)
                dset(d, s, D_SLEEP0, dur)
                add("sleep", "plain", s, first, b, d, r, ctr=ctr, dur=dur)
            b, d, r = fresh(s, first, "Splash")
            set_status(b, s, EXT | ctr)
            add("sleep", "extended", s, first, b, d, r, ctr=ctr, dur=0)
        # a sleeper on the bench too: a switch on the same turn carries both duration values along
        b, d, r = fresh(s, first, "Splash")
        set_status(b, s, 3)
        dset(d, s, D_SLEEP0, 2)
        _set_bench(b, s, 1)
        set_status(b, s, 4, pos=1)
        dset(d, s, (3, 3), 3)
        add("sleep", "switch", s, first, b, d, r, SWITCH_SEEDS, ctr=3, dur=2)
    # ---- confusion and disable: every counter with every duration value
    for s, first in each:
        for ctr in range(1, 8):
            for dur in range(1, 8):
                b, d, r = fresh(s, first, "Splash")
                _set_vlo(b, s, _vlo(b, s) | V["CONFUSION"])
                set_counter(b, s, 18, ctr)
                dset(d, s, D_CONFUSION, dur)
                add("confusion", "plain", s, first, b, d, r, SEEDS, ctr=ctr, dur=dur)
        for ctr in range(1, 16):
            for dur in range(1, 16):
                for kind in ("selected", "other"):
                    b, d, r = fresh(s, first, "Splash")
                    if kind == "other":
                        _set_move(b, s, 0, mid=move("Pound"))
                    set_disable(b, s, ctr, 1)
                    dset(d, s, D_DISABLE, dur)
                    add("disable", kind, s, first, b, d, r, ctr=ctr, dur=dur)
        for ctr in (1, 2, 5, 8):        # a disabled charging move: the turn is lost and the charge with it
            b, d, r = fresh(s, first, "SolarBeam")
            _set_vlo(b, s, _vlo(b, s) | V["CHARGING"])
            b[s * SIDE + LAST_SEL], b[LAST_MOVES + 2 * s] = move("SolarBeam"), 2
            set_disable(b, s, ctr, 2)
            dset(d, s, D_DISABLE, 1)
            set_hp(b, 1 - s, 999)
            add("disable", "charging", s, first, b, d, r, ctr=ctr, dur=1)
    # ---- thrash and binding
    for s, first in each:
        for name in ("Thrash", "PetalDance"):
            for ctr in range(1, 8):
                for dur in DURS:
                    b, d, r = fresh(s, first, name)
                    _set_vlo(b, s, _vlo(b, s) | V["THRASHING"])
                    set_counter(b, s, 21, ctr)
                    dset(d, s, D_ATTACKING, dur)
                    b[s * SIDE + LAST_SEL] = move(name)
                    set_hp(b, 1 - s, 999)
                    set_types(b, 1 - s, TYPES["Normal"], TYPES["Normal"])
                    add("thrash", name, s, first, b, d, r, SEEDS if ctr == 1 else 1, ctr=ctr, dur=dur)
        for ctr in range(1, 8):
            for dur in DURS:
                for last in BIND_DAMAGE:
                    for kind in ("bare", "substitute", "1 hp"):
                        b, d, r = fresh(s, first, "Wrap")
                        _set_vlo(b, s, _vlo(b, s) | V["BINDING"])
                        set_counter(b, s, 21, ctr)
                        dset(d, s, D_BINDING, dur)
                        b[s * SIDE + LAST_SEL] = move("Wrap")
                        put16(b, LAST_DAMAGE, last)
                        set_hp(b, 1 - s, 1 if kind == "1 hp" else 999, 999)
                        if kind == "substitute":
                            set_sub(b, 1 - s, 10)
                        add("binding", kind, s, first, b, d, r, ctr=ctr, dur=dur, last=last)
    # ---- every clock's first turn: the foe puts the subject to sleep, confuses it, disables a move; the subject thrashes and wraps
    for s, first in each:
        for kind, mine, foes in (("sleep", "Splash", "Spore"), ("confusion", "Splash", "ConfuseRay"), ("disable", "Splash", "Disable"),
                                 ("thrash", "Thrash", "Splash"), ("thrash", "PetalDance", "Splash"), ("binding", "Wrap", "Splash")):
            b, d, r = fresh(s, first, mine, foes)
            set_hp(b, 1 - s, 999)
            set_types(b, 1 - s, TYPES["Normal"], TYPES["Normal"])
            add("starts", kind, s, first, b, d, r, START_SEEDS, move=mine)
    # ---- flinch and recharge, alone and over a running confusion and a running disable
    for s, first in each:
        for bits in ("FLINCH", "RECHARGING", "FLINCH RECHARGING"):
            for over in ("nothing", "confusion", "disable"):
                b, d, r = fresh(s, first, "Splash")
                _set_vlo(b, s, _vlo(b, s) | sum(V[x] for x in bits.split()))
                if over == "confusion":
                    _set_vlo(b, s, _vlo(b, s) | V["CONFUSION"])
                    set_counter(b, s, 18, 3)
                    dset(d, s, D_CONFUSION, 2)
                elif over == "disable":
                    _set_move(b, s, 0, mid=move("Pound"))
                    set_disable(b, s, 4, 1)
                    dset(d, s, D_DISABLE, 2)
                add("flinch", bits, s, first, b, d, r, SEEDS if over == "confusion" else 1, over=over)
    # ---- a full paralysis and a confusion self-hit over each lock
    for s, first in each:
        for cause in ("paralysis", "confusion"):
            for lock, (bits, name, count, field) in LOCKS.items():
                b, d, r = fresh(s, first, name)
                _set_vlo(b, s, _vlo(b, s) | bits)
                set_counter(b, s, 21, count)
                if field is not None:
                    dset(d, s, (field, 3), 1)
                b[s * SIDE + LAST_SEL] = move(name)
                set_hp(b, 1 - s, 999)
                set_hp(b, s, 999)
                if cause == "paralysis":
                    set_status(b, s, PAR)
                else:
                    _set_vlo(b, s, _vlo(b, s) | V["CONFUSION"])
                    set_counter(b, s, 18, 3)
                    dset(d, s, D_CONFUSION, 1)
                add("locks", cause, s, first, b, d, r, 2 * SEEDS, lock=lock)
    return tuple(rows), tuple(tags), tuple(specs), tuple(reps)


def _stepped(b, d, r, p, max_steps):
    ob, od, op = b.copy(), d.copy(), p.copy()
    oout, osteps = O.rollout_batch(ob, od, r, op, max_steps=max_steps, threads=8)
    exp = dict(results=oout, steps=osteps, prng=op, battles=ob, durations=od)
    for a in exp.values():
        a.setflags(write=False)
    return exp


@functools.lru_cache(maxsize=None)
def cases():
    """Every lane: (battles, durations, results, prng, the oracle's turn-step of each, tag and spec per lane)."""
    rows, tags, specs, reps = states()
    n = np.array(reps)
    b = np.repeat(np.stack([x[0] for x in rows]), n, axis=0)
    d = np.repeat(np.stack([x[1] for x in rows]), n, axis=0)
    r = np.repeat(np.array([x[2] for x in rows], dtype=np.uint8), n)
    state = np.repeat(np.arange(len(rows)), n)
    b[:, RNG:RNG + 8] = np.random.default_rng(0xC10C).integers(0, 256, (len(b), 8), dtype=np.uint8)
    p = np.zeros((len(b), 8), dtype=np.uint8)
    O.LIB.oracle_fast_prng_seed_batch(O.ptr(p), len(p), C.c_uint64(0xC10CFFEE0000))
    exp = _stepped(b, d, r, p, 1)
    for a in (b, d, r, p):
        a.setflags(write=False)
    return b, d, r, p, exp, tuple(tags[k] for k in state), tuple(specs[k] for k in state)


@functools.lru_cache(maxsize=None)
def keyed():
    """The same turn-step of every lane once more through oracle_update, which also gives the 16-byte chance-action key, and both
    players' choices behind it: (P1's choice, P2's choice, actions, P1's next choices, P2's), the choices drawn as the rollout draws
    them.  It must reproduce cases()'s expectation byte for byte."""
    b, d, r, p, exp, tags, _ = cases()
    c1, c2, act = np.zeros(len(b), np.uint8), np.zeros(len(b), np.uint8), np.zeros((len(b), 16), np.uint8)
    nxt = [[], []]
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
        for pl in range(2):
            nxt[pl].append(O.choices(img, pl, (res >> (4 + 2 * pl)) & 3) if (res & 15) == 0 else None)
    for a in (c1, c2, act):
        a.setflags(write=False)
    return c1, c2, act, tuple(nxt[0]), tuple(nxt[1])


@functools.lru_cache(maxsize=None)
def queue_steps():
    """The oracle's QUEUE_STEPS (17) turn-steps of every lane of cases(): the clocks have to keep agreeing for sixteen more."""
    b, d, r, p, _, _, _ = cases()
    return _stepped(b, d, r, p, QUEUE_STEPS)


@functools.lru_cache(maxsize=None)
def one_roll():
    """Every lane's turn-step under the clamp to ONE damage roll (override byte 236 for both players, tests/damage_cases.py's
    roll_byte): (battles, durations, results, actions, P1's next choices, P2's)."""
    b, d, r, _, _, _, _ = cases()
    c1, c2, _, _, _ = keyed()
    ob, od = b.copy(), d.copy()
    ores, oact = np.zeros(len(b), np.uint8), np.zeros((len(b), 16), np.uint8)
    nxt = [[], []]
    opt = O.Options()
    over = np.zeros(16, np.uint8)
    over[0] = over[8] = 236
    for k in range(len(b)):
        opt.set(d[k], over)
        ores[k] = O.update(ob[k], int(c1[k]), int(c2[k]), opt)
        od[k], oact[k] = opt.durations, opt.actions
        for pl in range(2):
            nxt[pl].append(O.choices(ob[k], pl, (int(ores[k]) >> (4 + 2 * pl)) & 3) if (int(ores[k]) & 15) == 0 else None)
    for a in (ob, od, ores, oact):
        a.setflags(write=False)
    return ob, od, ores, oact, tuple(nxt[0]), tuple(nxt[1])
