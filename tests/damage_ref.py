"""The gen-1 damage arithmetic in plain integers: no oracle, no GPU, no battle image.  Written from the published formula (the
cartridge's, which Pokemon Showdown's gen-1 mod follows) so that oracle/gen1_engine.c and EngineR (oak_amd/csrc/gen1_regs.hpp), which
one author wrote, can both disagree with it.  tests/test_damage_ref.py holds the oracle to it.

The caller picks the operands: on a critical hit the UNMODIFIED (party) stats of both sides, otherwise the attacker's active stat and the
target's active stat, doubled when its screen (Reflect for a physical move, Light Screen for a special one) is up."""

SONIC_BOOM, DRAGON_RAGE, SEISMIC_TOSS, NIGHT_SHADE, SUPER_FANG, COUNTER, PSYWAVE = ("SonicBoom", "DragonRage", "SeismicToss", "NightShade",
                                                                                    "SuperFang", "Counter", "Psywave")


def scaled(atk, def_):
    """The one-byte stats the division works on: past 255 on either side both are quartered, kept to a byte and floored at 1."""
    if atk > 255 or def_ > 255:
        atk, def_ = max((atk // 4) & 255, 1), max((def_ // 4) & 255, 1)
    return atk, def_


def base(level, bp, atk, def_, crit, explode):
    atk, def_ = scaled(atk, def_)
    lvl = level * (2 if crit else 1)
    if explode:
        def_ = max(def_ // 2, 1)
    return min(((lvl * 2 // 5 + 2) * bp * atk // def_) // 50, 997) + 2


def capped(level, bp, atk, def_, crit, explode):
    """Did the quotient meet the cap of 997?"""
    atk, def_ = scaled(atk, def_)
    if explode:
        def_ = max(def_ // 2, 1)
    return ((level * (2 if crit else 1) * 2 // 5 + 2) * bp * atk // def_) // 50 >= 997


def adjust(d, stab, e1, e2, same_types):
    """Same-type bonus, then the target's first type, then its second when it is another: chart entries in halves, a truncation each."""
    if stab:
        d = (d + d // 2) & 0xFFFF
    if e1 != 2:
        d = (d * e1 // 2) & 0xFFFF
    if not same_types and e2 != 2:
        d = (d * e2 // 2) & 0xFFFF
    return d


def rolled(d, roll):
    """roll in 217 .. 255; damage of 0 or 1 is not rolled for."""
    return d if d <= 1 else d * roll // 255


def fixed(move, level, foe_hp, last_damage, draw):
    if move == SONIC_BOOM:
        return 20
    if move == DRAGON_RAGE:
        return 40
    if move in (SEISMIC_TOSS, NIGHT_SHADE):
        return level
    if move == SUPER_FANG:
        return max(foe_hp // 2, 1)
    if move == COUNTER:
        return min(2 * last_damage, 65535)
    if move == PSYWAVE:
        return draw
    raise ValueError(move)
