"""A numpy / plain-Python restatement of EngineR::inert_standstill (oak_amd/csrc/gen1_regs.hpp) on the 384-byte battle image, and the
fixture its tests share: long random OU playouts harvested from the CPU oracle.

`inert(b, d, result)` answers for ONE battle: is every further turn-step the same no-op, and if so how many battle.rng draws does
each make.  It is written from the engine's rules, not from the kernel's code, so that the two can disagree."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle_lib as O  # noqa: E402
from oak_amd import gamedata  # noqa: E402

SIDE, ACTIVE, ORDER, LAST_SEL, LAST_USED = 184, 144, 176, 182, 183
TURN, LAST_DAMAGE, LAST_MOVES, RNG = 368, 370, 372, 376
V = {n: 1 << i for i, n in enumerate(("BIDE", "THRASHING", "MULTIHIT", "FLINCH", "CHARGING", "BINDING", "INVULNERABLE", "CONFUSION", "MIST",
                                      "FOCUSENERGY", "SUBSTITUTE", "RECHARGING", "RAGE", "LEECHSEED", "TOXIC", "LIGHTSCREEN", "REFLECT",
                                      "TRANSFORM"))}
LOCKED = V["RECHARGING"] | V["RAGE"] | V["THRASHING"] | V["CHARGING"] | V["BIDE"]
BUSY = (V["FLINCH"] | V["RECHARGING"] | V["CONFUSION"] | V["BIDE"] | V["THRASHING"] | V["CHARGING"] | V["INVULNERABLE"] | V["MULTIHIT"] |
        V["BINDING"])
FRZ, PAR = 0x20, 0x40
M_COUNTER, M_QUICKATTACK, M_RAGE, M_STRUGGLE = 68, 98, 99, 165
_E = {n: i for i, n in enumerate(gamedata.EFFECT_NAMES)}
NOT_PLAIN = {_E[n] for n in ("SpecialDamage", "SuperFang", "OHKO", "Charge", "Metronome", "MirrorMove", "Thrashing", "Explode", "JumpKick")}
CHART = gamedata.DATA["type_chart"]
LCG_A, LCG_C, M64 = 0x5D588B656C078965, 0x269EC3, (1 << 64) - 1
RUNNING = 0x50   # result byte: nobody has won, both sides are asked for a move

assert gamedata.MOVE_NAMES[M_RAGE] == "Rage" and gamedata.MOVE_NAMES[M_STRUGGLE] == "Struggle" and gamedata.MOVE_NAMES[M_COUNTER] == "Counter"
assert gamedata.MOVE_NAMES[M_QUICKATTACK] == "QuickAttack"


def u16(b, o):
    return int(b[o]) | int(b[o + 1]) << 8


def u32(b, o):
    return u16(b, o) | u16(b, o + 2) << 16


def lcg(x, n):
    for _ in range(n):
        x = (LCG_A * x + LCG_C) & M64
    return x


def side_view(b, d, s):
    """What the predicate reads of side s: a dict of plain ints."""
    so = s * SIDE
    order = [int(v) for v in b[so + ORDER:so + ORDER + 6]]
    alive = [i != 0 and u16(b, so + (i - 1) * 24 + 18) > 0 for i in order]
    pk = so + (order[0] - 1) * 24 if order[0] else so
    vlo, vhi = u32(b, so + ACTIVE + 16), u32(b, so + ACTIVE + 20)
    moves = [(int(b[so + ACTIVE + 24 + 2 * i]), int(b[so + ACTIVE + 25 + 2 * i])) for i in range(4)]
    dur = u32(d, 4 * s)
    return dict(alive=alive, hp=u16(b, pk + 18) if order[0] else 0, status=int(b[pk + 20]) if order[0] else 0, vlo=vlo,
                disable_left=(vhi >> 20) & 15, disable_move=(vhi >> 24) & 7, moves=moves, spe=u16(b, so + ACTIVE + 6),
                types=int(b[so + ACTIVE + 11]), last_sel=int(b[so + LAST_SEL]), last_used=int(b[so + LAST_USED]),
                counterable=int(b[LAST_MOVES + 2 * s + 1]), dur_attacking=(dur >> 25) & 7, dur_binding=(dur >> 28) & 7)


def usable_moves(x):
    """Move slots the side may choose: in front of the first empty slot, with PP, not disabled."""
    out = []
    for i, (mid, pp) in enumerate(x["moves"]):
        if mid == 0:
            break
        if pp != 0 and x["disable_move"] != i + 1:
            out.append(i + 1)
    return out


def side_form(x, y, last_damage):
    """None, or (form, selected move or None when the choice is free, is it a PAR side that rolls)."""
    last = x["alive"][0] and not any(x["alive"][1:])
    locked = x["vlo"] & LOCKED
    struggle = not (x["vlo"] & (LOCKED | V["BINDING"])) and last and not usable_moves(x)
    sel = M_STRUGGLE if struggle else x["last_sel"] if locked else None
    if x["status"] == FRZ:
        if locked:
            return "frozen_locked", sel, False
        return ("frozen_free", sel, False) if last else None
    if x["status"] not in (0, PAR) or not (struggle or x["vlo"] & V["RAGE"]) or x["vlo"] & BUSY:
        return None
    if x["disable_left"] or x["disable_move"] or x["dur_attacking"] or x["dur_binding"]:
        return None
    eff, bp, mtype = gamedata.MOVES[sel - 1][:3]
    if bp == 0 or sel == M_COUNTER or eff in NOT_PLAIN:
        return None
    if CHART[mtype][y["types"] & 15] != 0 and CHART[mtype][y["types"] >> 4] != 0:
        return None
    par = x["status"] == PAR
    if x["last_used"] != sel or x["counterable"] != 0 or (par and last_damage != 0):
        return None
    return ("struggle" if struggle else "rage"), sel, par


def inert(b, d, result):
    """None, or (draws per turn-step, (form of side 1, form of side 2))."""
    if result != RUNNING or not 1 <= u16(b, TURN) < 1000:
        return None
    x, y = side_view(b, d, 0), side_view(b, d, 1)
    if not (x["alive"][0] and y["alive"][0]) or (x["vlo"] | y["vlo"]) & (V["BINDING"] | V["LEECHSEED"]):
        return None
    fx, fy = side_form(x, y, u16(b, LAST_DAMAGE)), side_form(y, x, u16(b, LAST_DAMAGE))
    if fx is None or fy is None:
        return None
    tie = 0
    if x["spe"] == y["spe"]:
        if fx[1] is None or fy[1] is None:
            return None
        tie = int((fx[1] == M_QUICKATTACK) == (fy[1] == M_QUICKATTACK) and (fx[1] == M_COUNTER) == (fy[1] == M_COUNTER))
    return tie + int(fx[2]) + int(fy[2]), (fx[0], fy[0])


@functools.lru_cache(maxsize=None)
def harvest(n=262144, at_step=300, threads=16):
    """Random OU playouts from the default seed base, advanced to `at_step` by the oracle, those still running kept: about 900
    states, a third of them stalemates and the rest ordinary long playouts (the negatives).  Returns read-only arrays
    (battles, durations, prng, results, total playout length by the oracle, the oracle's final result)."""
    b, d, p, r = O.make_random_ou_batch(n)
    res, steps = O.rollout_batch(b, d, r, p, max_steps=at_step, threads=threads)
    keep = np.where(((res & 15) == 0) & (steps == at_step))[0]
    b, d, p, res = b[keep].copy(), d[keep].copy(), p[keep].copy(), res[keep].copy()
    fb, fd, fp = b.copy(), d.copy(), p.copy()
    fres, fsteps = O.rollout_batch(fb, fd, res, fp, max_steps=1000 - at_step, threads=threads)
    out = (b, d, p, res, fsteps + at_step, fres)
    for a in out:
        a.setflags(write=False)
    return out
