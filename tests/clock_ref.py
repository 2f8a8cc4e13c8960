"""The gen-1 turn bookkeeping around a move in plain integers: no oracle, no GPU, no battle image.  Written from the published rules
(the cartridge's as Pokemon Showdown's gen-1 mod plays them, and the duration / observation bookkeeping of the chance-action key) so
that oracle/gen1_engine.c and EngineR (oak_amd/csrc/gen1_regs.hpp), which one author wrote, can both disagree with it.
tests/test_clock_ref.py holds the oracle to it.

A clock function takes the counter and the duration value and returns (next counter, does the Pokemon act, new duration, observation).
A function returns None where no game reaches the state and so no rule is published: a toxic counter stepping past 31, an extended
(Rest) sleep longer than 2, a disable count above 8, a confusion count above 5, a duration value that would leave its field.  Those
states are compared GPU-to-oracle only."""
FAILS = "fails"
STARTED, CONTINUING, ENDED = 1, 2, 3
# what a full paralysis and a confusion self-hit each take away
PARALYSIS_CLEARS = ("BIDE", "THRASHING", "CHARGING", "BINDING", "INVULNERABLE")
CONFUSION_CLEARS = PARALYSIS_CLEARS + ("MULTIHIT", "FLINCH")


def residual(max_hp, hp, status, toxic, toxic_ctr, seeded, foe_hp, foe_max):
    """status: "psn", "brn" or None; toxic: is the poison a Toxic one -> (hp, toxic_ctr, foe_hp)."""
    tick = max(1, max_hp // 16)
    for step in ("status", "seed"):
        if hp == 0 or not (seeded if step == "seed" else status in ("psn", "brn")):
            continue
        dmg = tick
        if toxic:
            toxic_ctr += 1
            if toxic_ctr > 31:
                return None
            dmg = tick * toxic_ctr
        hp = max(hp - dmg, 0)
        if step == "seed" and foe_hp > 0:
            foe_hp = min(foe_hp + dmg, foe_max)
    return hp, toxic_ctr, foe_hp


def heal(max_hp, hp, rest):
    """Recover / Soft-Boiled / Rest: the new HP (Rest: full, and the caller expects status `asleep, 2 turns, extended`, no toxic)."""
    if max_hp == hp or (max_hp - hp) % 256 == 255:
        return FAILS
    return max_hp if rest else min(hp + max_hp // 2, max_hp)


def substitute(max_hp, hp, has_one):
    cost = max_hp // 4
    if has_one or hp < cost:
        return FAILS
    return hp - cost, cost + 1


DRAWN = {"sleep": (1, 7), "confusion": (2, 5), "disable": (1, 8), "thrash": (2, 3), "binding": (1, 4)}   # a binding of 2 .. 5 turns in all


def started(clock, drawn):
    """The turn a clock starts: (counter, duration, observation); None for a length the clock is never drawn at."""
    return (drawn, 1, STARTED) if DRAWN[clock][0] <= drawn <= DRAWN[clock][1] else None


def flinch_recharge(flinch, recharging):
    """A flinch left standing from an earlier turn goes when a move is selected, and only a recharging Pokemon selects none; there the
    flinch costs the turn before the recharge is looked at, which then still stands.  No clock ticks on a turn lost to either.
    -> (acts, flinch after, recharging after)"""
    return (False, False, bool(flinch)) if recharging else (True, False, False)


def _tick(ctr, dur, field, most):
    """One step of a counter with a duration value in a `field`-bit field: (next counter, new duration, observation)."""
    if not 1 <= ctr <= most or (ctr > 1 and dur + 1 >= 1 << field):
        return None
    return (0, 0, ENDED) if ctr == 1 else (ctr - 1, dur + 1, CONTINUING)


def sleep(ctr, dur, extended):
    """The waking turn is lost.  A Rest sleep is not observed: its duration value and the key stay as they are."""
    if extended:
        return (ctr - 1, False, dur, 0) if 1 <= ctr <= 2 else None
    t = _tick(ctr, dur, 3, 7)
    return t and (t[0], False, t[1], t[2])


def confusion(ctr, dur, hits_self):
    """hits_self: the 128/256 draw, made only while the confusion goes on."""
    t = _tick(ctr, dur, 3, 5)
    return t and (t[0], t[0] == 0 or not hits_self, t[1], t[2])


def disable(ctr, dur, selected_is_disabled):
    """A disabled selected move costs the turn (and drops a charge); the turn the count ends nothing is disabled any more."""
    t = _tick(ctr, dur, 4, 8)
    return t and (t[0], t[0] == 0 or not selected_is_disabled, t[1], t[2])


def thrash(ctr, dur, drawn):
    """Thrash / Petal Dance attack every turn; the last one starts a confusion of `drawn` (2 .. 5) turns:
    (..., confusion counter, confusion duration, confusion observation) follow the usual four."""
    t = _tick(ctr, dur, 3, 7)
    if t is None or (t[0] == 0 and not 2 <= drawn <= 5):
        return None
    return (t[0], True, t[1], t[2]) + ((drawn, 1, STARTED) if t[0] == 0 else (0, 0, 0))


def binding(ctr, dur, last_damage, foe_hp, foe_sub):
    """The binder's turn: the foe cannot move, the binder repeats last_damage (into a substitute where one stands) and the duration is
    observed as continuing; a counter that reaches 0 lets go at the end of the turn, a foe that faints is let go at once.
    -> (next counter, still binding, new duration, observation, foe_hp, foe_sub or 0 when it broke)."""
    if foe_sub and last_damage:
        foe_sub = max(foe_sub - last_damage, 0)
    else:
        foe_hp -= min(last_damage, foe_hp)
    holds = ctr > 1 and foe_hp > 0
    if not 1 <= ctr <= 7 or (holds and dur + 1 >= 8):
        return None
    return ctr - 1, holds, dur + 1 if holds else 0, CONTINUING, foe_hp, foe_sub
