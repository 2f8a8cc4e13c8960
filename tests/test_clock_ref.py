"""The CPU oracle's turn bookkeeping (oracle/gen1_engine.c: before_move, handle_residual, faint / check_faint and on_begin's Heal and
Substitute) against tests/clock_ref.py, a restatement in plain integers that shares no code with it, on the constructed states of
tests/clock_cases.py; and the conditions under which those states are worth running on the GPU (tests/test_gpu_clock_edges.py).
No GPU.

Whether the subject ACTED is read off the image, never off the oracle's control flow: a move that executes costs a PP (Thrash's later
turns and a fired charge move are told by the HP the foe lost), a lost turn costs none.

Compared GPU-to-oracle only, because no game reaches them and so no rule is published (clock_ref returns None): a toxic counter
stepping from 31 to 0, an extended (Rest) sleep of 3 .. 7, a disable count above 8, a confusion count above 5, and a duration value in
the last value of its field that would have to grow again."""
import collections

import numpy as np

import clock_cases as K
import clock_ref as R
from inert_ref import ACTIVE, SIDE, V
from test_gpu_choice_draw import _vlo

ERROR = 4
HP0 = 999      # what a foe that a case is not about starts from


def _key(act, s):
    """The observations of player s from the 16-byte action key: two-bit flags are 0 not rolled, 1 false, 2 true."""
    w = int.from_bytes(bytes(act[8 * s:8 * s + 8]), "little")
    return dict(hit=(w >> 8) & 3, confused=(w >> 16) & 3, paralyzed=(w >> 18) & 3, sleep=(w >> 24) & 3, confusion=(w >> 26) & 7,
                disable=(w >> 29) & 3, attacking=(w >> 31) & 3, binding=(w >> 33) & 7)


def _switched(b, ob, s):
    return int(b[s * SIDE + 176]) != int(ob[s * SIDE + 176])


def _old(b, ob, s):
    """The order position at which the turn-step left the Pokemon that was active before it."""
    return [int(x) for x in ob[s * SIDE + 176:s * SIDE + 182]].index(int(b[s * SIDE + 176]))


class Lane:
    """One lane before (b, d) and after (ob, od) the oracle's turn-step, the subject s and its key."""

    def __init__(self, k, data):
        b, d, _, _, exp, tags, specs = data[0]
        self.b, self.d, self.ob, self.od = b[k], d[k], exp["battles"][k], exp["durations"][k]
        self.result = int(exp["results"][k])
        self.spec, self.tag = specs[k], tags[k]
        self.s = specs[k]["s"]
        self.f = 1 - self.s
        self.key = _key(data[1][2][k], self.s)
        self.seen = data[2]

    def bit(self, name, after=True, side=None):
        return bool(_vlo(self.ob if after else self.b, self.s if side is None else side) & V[name])

    def spent(self, side=None):
        """PP the side spent in the turn-step."""
        side = self.s if side is None else side
        return K.pp_sum(self.b, side) - K.pp_sum(self.ob, side)


def _residual(x, hp=None, status=None, toxic=None):
    """Assert the holder's residual damage of this turn-step, given its HP, status byte and Toxic bit when its own move was done with
    (by default what they were before the turn-step).  Returns what happened, for the coverage conditions."""
    s, f, b, ob = x.s, x.f, x.b, x.ob
    hp = K.hp_of(b, s) if hp is None else hp
    st = K.status_at(b, s) if status is None else status
    toxic = x.bit("TOXIC", after=False) if toxic is None else toxic
    name = "brn" if st & K.BRN else "psn" if st & K.PSN and not st & 7 else None
    ctr, seeded = K.toxic_ctr(b, s) if toxic else 0, x.bit("LEECHSEED", after=False)
    pos = _old(ob, b, f)                 # the foe the residual meets: the one active AFTER the foe's own action, as it was before
    foe_hp, foe_max = K.hp_of(b, f, pos), K.max_hp_of(b, f, pos)
    if foe_hp == 0:                      # a foe without HP ends the turn before any residual
        assert K.hp_of(ob, s) == hp and (K.toxic_ctr(ob, s) == ctr or not toxic), "a residual ran over a fainted foe"
        return "none"
    max_hp = K.max_hp_of(b, s)
    want = R.residual(max_hp, hp, name, toxic, ctr, seeded, foe_hp, foe_max)
    if want is None:
        return "compared only"
    assert (K.hp_of(ob, s), K.hp_of(ob, f)) == (want[0], want[2]), ("hp", K.hp_of(ob, s), K.hp_of(ob, f), want)
    if want[0] > 0:
        assert K.toxic_ctr(ob, s) == (want[1] if toxic else 0), ("toxic counter", K.toxic_ctr(ob, s), want)
    else:                                # fainted: every volatile and the status go
        assert _vlo(ob, s) == 0 and K.status_at(ob, s) == 0
    tick = max(1, max_hp // 16)
    mid = R.residual(max_hp, hp, name, toxic, ctr, False, foe_hp, foe_max)       # the state between the two steps
    out = {"floor"} if max_hp < 16 and (name or seeded) else set()
    if name and mid[0] == 0:
        out.add("faint by the tick")
    elif seeded:
        if want[0] == 0:
            out.add("faint by the seed")
        out.add("capped heal" if want[2] - foe_hp < tick * (want[1] if toxic else 1) else "uncapped heal")
    x.seen["residual", s] |= out
    return "ran"


def check_residual(x):
    sp, s, f, b, ob = x.spec, x.s, x.f, x.b, x.ob
    kind = sp["kind"]
    if kind == "switch" and _switched(b, ob, s):
        pos = _old(b, ob, s)
        assert K.hp_of(ob, s, pos) == 100 and K.status_at(ob, s, pos) == K.PSN and K.hp_of(ob, f) == 500 and _vlo(ob, s) == 0
        x.seen["switched", s].add(sp["status"])
        return
    if kind == "faints the foe":
        assert K.hp_of(ob, f) == 0 and K.hp_of(ob, s) == 100 and K.toxic_ctr(ob, s) == (sp["ctr"] or 0) and x.result & 15 in (1, 2)
        return
    how = _residual(x)
    if kind == "grid":
        x.seen["cells", how].add(x.tag)
        assert (how == "none") == (sp["foe_hp"] == 0 and not _switched(b, ob, f)), how
        if how == "compared only":
            assert sp["status"] == "tox" and sp["ctr"] + 1 + sp["seeded"] > 31
    else:
        assert how == "ran"
    if kind == "switch":
        x.seen["stayed", s].add(sp["status"])


def check_heal(x):
    sp, s, b, ob, d, od = x.spec, x.s, x.b, x.ob, x.d, x.od
    max_hp, hp, rest = sp["max_hp"], sp["max_hp"] - sp["lost"], sp["kind"] == "Rest"
    if sp["status"] == "par":
        assert x.key["paralyzed"] in (1, 2)
        x.seen["rest par", s].add(x.key["paralyzed"])
    stopped = x.key["paralyzed"] == 2
    want = R.FAILS if stopped else R.heal(max_hp, hp, rest)
    assert x.spent() == (0 if stopped else 1)
    stats = slice(s * SIDE + ACTIVE + 2, s * SIDE + ACTIVE + 10)
    assert (b[stats] == ob[stats]).all(), "Rest gives no stat back"
    if want == R.FAILS:
        if not stopped:
            x.seen["heal fails", s].add("full" if sp["lost"] == 0 else sp["lost"])
        assert K.dget(od, s, K.D_SLEEP0) == 5
        assert _residual(x) == "ran"          # (which also says: HP, status and the Toxic state are what they were)
        assert K.status_at(ob, s) == K.status_at(b, s)
        return
    x.seen["heal works", s].add("rest" if rest else "capped" if hp + max_hp // 2 > max_hp else "all of it")
    assert K.hp_of(ob, s) == want, (K.hp_of(ob, s), want)
    if rest:
        assert K.status_at(ob, s) == K.EXT | 2 and not x.bit("TOXIC") and K.toxic_ctr(ob, s) == 0 and K.dget(od, s, K.D_SLEEP0) == 0
        x.seen["rest under", s].add(sp["status"])
    else:
        assert K.status_at(ob, s) == 0 and K.dget(od, s, K.D_SLEEP0) == 5


def check_substitute(x):
    sp, s, b, ob = x.spec, x.s, x.b, x.ob
    if _switched(b, ob, s):
        return
    want = R.substitute(sp["max_hp"], sp["hp"], sp["has_one"])
    assert x.spent() == 1
    if want == R.FAILS:
        x.seen["substitute", s].add("has one" if sp["has_one"] else "too little")
        assert K.hp_of(ob, s) == sp["hp"] and x.bit("SUBSTITUTE") == bool(sp["has_one"]) and K.sub_hp(ob, s) == (7 if sp["has_one"] else 0)
        return
    assert K.hp_of(ob, s) == want[0], (K.hp_of(ob, s), want)
    if want[0] == 0:        # exactly a quarter: the user faints; with somebody on the bench it is asked to switch, else it has lost
        x.seen["substitute", s].add("faints, " + sp["kind"])
        asked = (x.result >> (4 + 2 * s)) & 3
        assert (x.result & 15, asked) == ((0, 2) if sp["kind"] == "bench" else (2 - s, 0)), hex(x.result)
        assert _vlo(ob, s) == 0
    else:
        x.seen["substitute", s].add("free" if sp["max_hp"] < 4 else "stands")
        assert x.bit("SUBSTITUTE") and K.sub_hp(ob, s) == want[1], (K.sub_hp(ob, s), want)


def _sleep(x, ctr, dur, extended):
    want = R.sleep(ctr, dur, extended)
    if want is None:
        return False
    s = x.s
    assert K.status_at(x.ob, s) == (0 if want[0] == 0 else (K.EXT if extended else 0) | want[0]), K.status_at(x.ob, s)
    assert K.dget(x.od, s, K.D_SLEEP0) == want[2] and x.key["sleep"] == want[3], (K.dget(x.od, s, K.D_SLEEP0), x.key["sleep"], want)
    assert x.spent() == 0, "a sleeper acted (the waking turn is lost too)"
    if not extended:
        x.seen["sleep", s].add((ctr, want[3]))
    return True


def check_sleep(x):
    sp, s = x.spec, x.s
    if sp["kind"] == "switch":
        if _switched(x.b, x.ob, s):      # both duration values go with their Pokemon, and nothing ticked
            assert (K.dget(x.od, s, K.D_SLEEP0), K.dget(x.od, s, (3, 3))) == (3, 2) and K.status_at(x.ob, s) == 4 and K.status_at(x.ob, s, 1) == 3
            assert int(x.od.view(np.uint32)[s]) >> 18 == 0
            x.seen["sleep switch", s].add(True)
            return
        x.seen["sleep switch", s].add(False)
        assert K.dget(x.od, s, (3, 3)) == 3 and K.status_at(x.ob, s, 1) == 4
    held = _sleep(x, sp["ctr"], sp["dur"], sp["kind"] == "extended")
    assert held == (not (sp["kind"] == "extended" and sp["ctr"] > 2)), sp


def _confusion(x, ctr, dur, family="confusion"):
    """The confusion clock of a subject that gets as far as it: returns (held by the referee, does the subject go on to its move)."""
    s, hits = x.s, x.key["confused"] == 2
    want = R.confusion(ctr, dur, hits)
    if want is None:
        return False, None
    assert (x.key["confused"] != 0) == (want[0] > 0), "the self-hit is drawn for exactly while the confusion goes on"
    assert (K.conf_left(x.ob, s), x.bit("CONFUSION")) == (want[0], want[0] > 0), (K.conf_left(x.ob, s), want)
    assert K.dget(x.od, s, K.D_CONFUSION) == want[2] and x.key["confusion"] == want[3], (K.dget(x.od, s, K.D_CONFUSION), x.key["confusion"], want)
    if not want[1]:
        assert K.hp_of(x.ob, s) < K.hp_of(x.b, s), "a self-hit that cost nothing"
    x.seen[family, s].add((ctr, want[3]))
    if want[0] > 0:
        x.seen[family + " draw", s].add((ctr, hits))
    return True, want[1]


def _disable(x, ctr, dur, selected):
    s = x.s
    want = R.disable(ctr, dur, selected)
    if want is None:
        return False, None
    slot = K.disable_of(x.b, s)[1]
    assert K.disable_of(x.ob, s) == (want[0], slot if want[0] else 0), (K.disable_of(x.ob, s), want)
    assert K.dget(x.od, s, K.D_DISABLE) == want[2] and x.key["disable"] == want[3], (K.dget(x.od, s, K.D_DISABLE), x.key["disable"], want)
    x.seen["disable", s].add((ctr, want[3]))
    return True, want[1]


def check_confusion(x):
    held, acts = _confusion(x, x.spec["ctr"], x.spec["dur"])
    assert held == (x.spec["ctr"] <= 5 and not (x.spec["ctr"] > 1 and x.spec["dur"] == 7)), x.spec
    if held:
        assert x.spent() == int(acts)


def check_disable(x):
    sp = x.spec
    held, acts = _disable(x, sp["ctr"], sp["dur"], sp["kind"] != "other")
    assert held == (sp["ctr"] <= 8 and not (sp["ctr"] > 1 and sp["dur"] == 15)), sp
    if not held:
        return
    x.seen["disabled", x.s].add((sp["kind"], acts))
    assert x.spent() == int(acts)
    if sp["kind"] == "charging":           # a charge that fires costs its PP then; a disabled one is dropped
        assert not x.bit("CHARGING") and (K.hp_of(x.ob, x.f) < HP0) == acts


def check_thrash(x):
    sp, s = x.spec, x.s
    drawn = K.conf_left(x.ob, s)
    if sp["ctr"] == 1:
        assert 2 <= drawn <= 5, drawn
        x.seen["thrash length", s].add(drawn)
    want = R.thrash(sp["ctr"], sp["dur"], drawn)
    assert (want is None) == (sp["ctr"] > 1 and sp["dur"] == 7)
    if want is None:
        return
    assert (K.attacks(x.ob, s), x.bit("THRASHING")) == (want[0], want[0] > 0), (K.attacks(x.ob, s), want)
    assert K.dget(x.od, s, K.D_ATTACKING) == want[2] and x.key["attacking"] == want[3], (K.dget(x.od, s, K.D_ATTACKING), x.key["attacking"], want)
    assert K.hp_of(x.ob, x.f) < HP0 and x.spent() == 0, "every turn of a Thrash attacks, and only the first costs a PP"
    assert (K.conf_left(x.ob, s), x.bit("CONFUSION"), K.dget(x.od, s, K.D_CONFUSION), x.key["confusion"]) == (want[4], want[4] > 0, want[5], want[6])
    x.seen["thrash", s].add((sp["ctr"], want[3]))


def check_binding(x):
    sp, s, f = x.spec, x.s, x.f
    sub = 10 if sp["kind"] == "substitute" else 0
    want = R.binding(sp["ctr"], sp["dur"], sp["last"], 1 if sp["kind"] == "1 hp" else HP0, sub)
    if want is None:
        assert sp["ctr"] > 1 and sp["dur"] == 7
        return
    assert x.spent() == 0 and x.spent(f) == 0, "a bound foe cannot move, and the binder repeats without a PP"
    assert (K.hp_of(x.ob, f), K.sub_hp(x.ob, f), x.bit("SUBSTITUTE", side=f)) == (want[4], want[5], want[5] > 0), (K.hp_of(x.ob, f), K.sub_hp(x.ob, f), want)
    assert (x.bit("BINDING"), K.dget(x.od, s, K.D_BINDING), x.key["binding"]) == want[1:4], (x.bit("BINDING"), K.dget(x.od, s, K.D_BINDING), want)
    if want[4] > 0:
        assert K.attacks(x.ob, s) == want[0]
    x.seen["binding", s].add((sp["ctr"], want[3], "let go" if not want[1] else "holds"))
    x.seen["binding into", s].add((sp["kind"], "nothing" if sp["last"] == 0 else "breaks" if sub and not want[5] else "faints" if not want[4] else "hurts"))


def check_starts(x):
    sp, s, f, first = x.spec, x.s, x.f, x.spec["first"]
    kind = sp["kind"]
    if kind == "thrash":
        want = R.started("thrash", K.attacks(x.ob, s))
        assert want and x.bit("THRASHING") and (K.dget(x.od, s, K.D_ATTACKING), x.key["attacking"]) == want[1:], (K.attacks(x.ob, s), want)
        assert x.spent() == 1 and K.hp_of(x.ob, f) < HP0
        x.seen["thrash", s].add((want[0], want[2]))
    elif kind == "binding":
        assert x.key["hit"] in (1, 2) and x.bit("BINDING") == (x.key["hit"] == 2)
        if x.key["hit"] == 2:
            want = R.started("binding", K.attacks(x.ob, s))
            assert want and (K.dget(x.od, s, K.D_BINDING), x.key["binding"]) == want[1:], (K.attacks(x.ob, s), want)
            assert x.spent() == 1 and K.hp_of(x.ob, f) < HP0 and x.spent(f) == (0 if first else 1)
            x.seen["binding", s].add((want[0], want[2], "holds"))
        else:
            assert K.dget(x.od, s, K.D_BINDING) == 0 and x.key["binding"] == 0
    elif kind == "sleep":
        # the subject that acts first is asleep with the drawn counter; the one that acts second has slept one turn of it already
        left = K.status_at(x.ob, s)
        if first:
            want = R.started("sleep", left)
            assert want and (K.dget(x.od, s, K.D_SLEEP0), x.key["sleep"]) == want[1:] and x.spent() == 1
            x.seen["sleep", s].add((want[0], want[2]))
        else:
            n = left + 1 if left else 1
            assert R.started("sleep", n) and _sleep(x, n, 1, False)
    elif kind == "confusion":
        if first:
            want = R.started("confusion", K.conf_left(x.ob, s))
            assert want and x.bit("CONFUSION") and (K.dget(x.od, s, K.D_CONFUSION), x.key["confusion"]) == want[1:] and x.spent() == 1
            x.seen["confusion", s].add((want[0], want[2]))
        else:
            n = K.conf_left(x.ob, s) + 1
            assert R.started("confusion", n)
            held, acts = _confusion(x, n, 1)
            assert held and x.spent() == int(acts)
    else:
        assert x.key["disable"] == 0 or _key_hit(x, f) == 2
        if _key_hit(x, f) != 2:
            assert K.disable_of(x.ob, s) == (0, 0) and K.dget(x.od, s, K.D_DISABLE) == 0 and x.spent() == 1
        elif first:
            left, slot = K.disable_of(x.ob, s)
            want = R.started("disable", left)
            assert want and 1 <= slot <= 4 and (K.dget(x.od, s, K.D_DISABLE), x.key["disable"]) == want[1:] and x.spent() == 1
            x.seen["disable", s].add((want[0], want[2]))
        else:
            left, slot = K.disable_of(x.ob, s)
            n = left + 1
            assert R.started("disable", n)
            want = R.disable(n, 1, True)       # all four slots hold the one move: whichever is disabled, the selected move is
            assert (left, K.dget(x.od, s, K.D_DISABLE), x.key["disable"]) == (want[0], want[2], want[3]) and (slot != 0) == (left != 0)
            assert x.spent() == int(want[1])
            x.seen["disable", s].add((n, want[3]))


def _key_hit(x, side):
    return _key(x.act, side)["hit"]


def check_flinch(x):
    sp, s = x.spec, x.s
    flinch, recharging = "FLINCH" in sp["kind"], "RECHARGING" in sp["kind"]
    acts, flinch_after, recharging_after = R.flinch_recharge(flinch, recharging)
    assert (x.bit("FLINCH"), x.bit("RECHARGING")) == (flinch_after, recharging_after)
    if sp["over"] == "confusion":
        if acts:
            held, acts = _confusion(x, 3, 2, "confusion under a flinch")
            assert held
        else:
            assert (K.conf_left(x.ob, s), K.dget(x.od, s, K.D_CONFUSION), x.key["confusion"], x.key["confused"]) == (3, 2, 0, 0)
    elif sp["over"] == "disable":
        if acts:
            held, acts = _disable(x, 4, 2, False)
            assert held
        else:
            assert (K.disable_of(x.ob, s), K.dget(x.od, s, K.D_DISABLE), x.key["disable"]) == ((4, 1), 2, 0)
    assert x.spent() == int(acts)
    x.seen["flinch", s].add((sp["kind"], sp["over"]))


def check_locks(x):
    sp, s = x.spec, x.s
    bits, _, count, field = K.LOCKS[sp["lock"]]
    if sp["kind"] == "paralysis":
        assert x.key["paralyzed"] in (1, 2)
        lost, clears = x.key["paralyzed"] == 2, R.PARALYSIS_CLEARS
    else:
        held, acts = _confusion(x, 3, 1, "confusion over a lock")
        assert held
        lost, clears = not acts, R.CONFUSION_CLEARS
    x.seen["locks", s].add((sp["kind"], sp["lock"], lost))
    if not lost:
        return
    gone = sum(V[n] for n in clears)
    before, after = _vlo(x.b, s) & 0x3FFFF, _vlo(x.ob, s) & 0x3FFFF
    assert after == before & ~gone, (hex(before), hex(after))
    assert K.dget(x.od, s, K.D_ATTACKING) == 0 and K.dget(x.od, s, K.D_BINDING) == 0 and x.key["attacking"] == 0 and x.key["binding"] == 0
    assert x.spent() == 0 and K.hp_of(x.ob, x.f) == HP0 and (K.hp_of(x.ob, s) == HP0) == (sp["kind"] == "paralysis")


CHECKS = dict(residual=check_residual, heal=check_heal, substitute=check_substitute, sleep=check_sleep, confusion=check_confusion,
              disable=check_disable, thrash=check_thrash, binding=check_binding, starts=check_starts, flinch=check_flinch, locks=check_locks)
_DATA = []


def _checked():
    """Every lane checked against the referee once: the record of what was seen, for the coverage conditions."""
    if not _DATA:
        data = (K.cases(), K.keyed(), collections.defaultdict(set))
        for k in range(len(data[0][0])):
            x = Lane(k, data)
            x.act = data[1][2][k]
            try:
                CHECKS[x.spec["family"]](x)
            except AssertionError as e:
                raise AssertionError((x.tag,) + e.args) from None
        _DATA.append(data[2])
    return _DATA[0]


def test_the_oracle_keeps_the_clocks_as_clock_ref_does():
    b, d, r, p, exp, tags, specs = K.cases()
    assert ((exp["results"] & 15) != ERROR).all() and (exp["steps"] == 1).all()
    assert {t[0] for t in tags} == set(K.FAMILIES) == set(CHECKS)
    assert len(b) <= 40000
    _checked()


def test_the_residual_cases_reach_what_they_are_built_for():
    seen = _checked()
    _, tags, _, _ = K.states()
    grid = {t for t in tags if t[:2] == ("residual", "grid")}
    ran, none, compared = seen["cells", "ran"], seen["cells", "none"], seen["cells", "compared only"]
    assert ran | none | compared == grid
    # every cell with a foe that has HP was reached, but for the toxic counter's wrap; a foe at 0 HP saw both a turn that ended there and
    # a replacement that the residual then met
    foe0 = {t for t in grid if t[-1] == 0}
    assert ran | compared >= grid - foe0 and none <= foe0 and ran & foe0 and none
    # (a counter of 30 under a seed never gets to step twice: 31 sixteenths are more than anybody has)
    assert {t[5:8] for t in compared} == {("tox", 31, 0), ("tox", 31, 1)}, sorted({t[5:8] for t in compared})
    for s in range(2):
        assert seen["residual", s] == {"floor", "faint by the tick", "faint by the seed", "capped heal", "uncapped heal"}, (s, seen["residual", s])
        assert seen["switched", s] == seen["stayed", s] == {"psn", "tox"}, (s, seen["switched", s], seen["stayed", s])
        assert seen["sleep switch", s] == {False, True}


def test_every_counter_value_started_went_on_and_ended_for_both_players():
    seen = _checked()
    S, C, E = R.STARTED, R.CONTINUING, R.ENDED
    for s in range(2):
        want = {(n, S) for n in range(1, 8)} | {(n, C) for n in range(2, 8)} | {(1, E)}
        assert seen["sleep", s] == want, (s, "sleep", sorted(want ^ seen["sleep", s]))
        want = {(n, S) for n in range(2, 6)} | {(n, C) for n in range(2, 6)} | {(1, E)}
        assert seen["confusion", s] == want, (s, "confusion", sorted(want ^ seen["confusion", s]))
        want = {(n, S) for n in range(1, 9)} | {(n, C) for n in range(2, 9)} | {(1, E)}
        assert seen["disable", s] == want, (s, "disable", sorted(want ^ seen["disable", s]))
        want = {(n, S) for n in (2, 3)} | {(n, C) for n in range(2, 8)} | {(1, E)}
        assert seen["thrash", s] == want, (s, "thrash", sorted(want ^ seen["thrash", s]))
        want = {(n, S, "holds") for n in range(1, 5)} | {(n, C, "holds") for n in range(2, 8)} | {(n, C, "let go") for n in range(1, 8)}
        assert seen["binding", s] == want, (s, "binding", sorted(want ^ seen["binding", s]))
        into = {(k, "nothing") for k in ("bare", "substitute", "1 hp")} | {("bare", "hurts"), ("substitute", "hurts"), ("substitute", "breaks"), ("1 hp", "faints"), ("bare", "faints")}
        assert seen["binding into", s] == into, (s, sorted(into ^ seen["binding into", s]))
        assert seen["disabled", s] == {("selected", False), ("selected", True), ("other", True), ("charging", False), ("charging", True)}
        assert len(seen["flinch", s]) == 9


def test_both_outcomes_of_every_draw_at_every_counter_value():
    seen = _checked()
    for s in range(2):
        want = {(n, hits) for n in range(2, 6) for hits in (False, True)}
        assert seen["confusion draw", s] == want, (s, sorted(want ^ seen["confusion draw", s]))
        assert seen["thrash length", s] == {2, 3, 4, 5}, (s, seen["thrash length", s])
        want = {(c, lock, lost) for c in ("paralysis", "confusion") for lock in K.LOCKS for lost in (False, True)}
        assert seen["locks", s] == want, (s, sorted(want ^ seen["locks", s]))
        assert seen["confusion under a flinch draw", s] == {(3, False), (3, True)}
        assert seen["rest par", s] == {1, 2}


def test_every_way_a_heal_and_a_substitute_fail_and_work():
    seen = _checked()
    for s in range(2):
        assert seen["heal fails", s] == {"full", 255, 511, 767}, (s, seen["heal fails", s])
        assert seen["heal works", s] == {"rest", "capped", "all of it"}, (s, seen["heal works", s])
        assert seen["rest under", s] == {None, "psn", "tox", "brn", "par"}, (s, seen["rest under", s])
        assert seen["substitute", s] == {"has one", "too little", "faints, alone", "faints, bench", "free", "stands"}, (s, seen["substitute", s])


def test_the_oracle_plays_every_case_on_to_the_queue_kernels_cap():
    b, d, r, p, exp, tags, _ = K.cases()
    far = K.queue_steps()
    assert ((far["results"] & 15) != ERROR).all() and (far["steps"] >= 1).all() and (far["steps"] <= K.QUEUE_STEPS).all()
    assert (far["steps"] == K.QUEUE_STEPS).sum() > len(b) // 4
