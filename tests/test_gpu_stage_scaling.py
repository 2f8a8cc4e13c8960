"""EngineR::scale_boost (one multiply against the stage table, oak_amd/csrc/gen1_regs.hpp) against the CPU oracle: exactly ONE turn-step
of edited states, byte for byte.

  accuracy / evasion: every stage -6 .. +6 of the mover's accuracy crossed with every stage of the foe's evasion, for one move of each
      accuracy byte 255, 229, 216, 191, 178, 140 and 76 (all four slots of BOTH sides hold the move and neither has anybody to switch
      to; P2 runs the transposed pair of stages), under SEEDS choice streams.  The oracle's side alone shows that at every stage of
      either kind the move both lands and fails wherever the rules leave both open -- for six of the seven: accuracy 76 belongs to the
      one-hit KO moves alone, which carry no base power in the move table and change nothing in oracle and engine alike; they are
      compared like the rest.
  stat stages: every move of gen 1 that raises or lowers a stat -- by one and by two where the game has such a move, the secondary
      effects included (Special falls only through one; nothing raises Speed by one or lowers Attack, Speed or Special by two) --
      from every stage of that stat, on unmodified stats 1, 2, 3, 4, 99, 100, 101, 255, 256, 499, 500, 998 and 999 (the cap of 999, the
      floor of 1 and the boundaries of the divisions by 100 and by 10).

The launches are small and run with the lane spread off, like tests/test_gpu_choice_draw.py's, whose base states these are."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
from inert_ref import ACTIVE, SIDE, V, u16, u32
from oak_amd import gamedata
from test_gpu_choice_draw import _bases, _compare, _set_bench, _set_move, _spread, _stored, _vlo

SEEDS = 4
STAGES = range(-6, 7)
ACCURACY_MOVES = {255: "Pound", 229: "RockSlide", 216: "MegaPunch", 191: "Slam", 178: "Thunder", 140: "Supersonic", 76: "HornDrill"}
STATS = (1, 2, 3, 4, 99, 100, 101, 255, 256, 499, 500, 998, 999)
# effect -> (the stat: 0 atk 1 def 2 spe 3 spc, stages, on the user?)
STAGE_EFFECTS = {"AttackUp1": (0, 1, True), "AttackUp2": (0, 2, True), "DefenseUp1": (1, 1, True), "DefenseUp2": (1, 2, True),
                 "SpeedUp2": (2, 2, True), "SpecialUp1": (3, 1, True), "SpecialUp2": (3, 2, True),
                 "AttackDown1": (0, -1, False), "DefenseDown1": (1, -1, False), "DefenseDown2": (1, -2, False), "SpeedDown1": (2, -1, False),
                 "AttackDownChance": (0, -1, False), "DefenseDownChance": (1, -1, False), "SpeedDownChance": (2, -1, False),
                 "SpecialDownChance": (3, -1, False)}
RATIOS = [tuple(r) for r in gamedata.DATA["boosts"]]


def _move(name):
    return gamedata.MOVE_NAMES.index(name)


def _stage_moves():
    """One move per stat-stage effect: the first that has it."""
    out = {}
    for mid in range(1, len(gamedata.MOVE_NAMES)):
        eff = gamedata.EFFECT_NAMES[gamedata.MOVES[mid - 1][0]]
        if eff in STAGE_EFFECTS and eff not in out:
            out[eff] = mid
    assert set(out) == set(STAGE_EFFECTS), sorted(set(STAGE_EFFECTS) - set(out))
    return out


def _set_stage(b, s, idx, stage):
    """Nibble idx (0 atk 1 def 2 spe 3 spc 4 acc 5 eva) of the active Pokemon's boosts: a 4-bit two's complement stage."""
    o = s * SIDE + ACTIVE + 12 + idx // 2
    sh = 4 * (idx % 2)
    b[o] = (int(b[o]) & ~(15 << sh)) | ((stage & 15) << sh)


def _scaled(x, stage):
    num, den = RATIOS[stage + 6]
    return x * num // den


def _all_slots(b, s, mid):
    for i in range(4):
        _set_move(b, s, i, mid=mid, pp=10)


def _clean(b, k):
    """Neither active Pokemon has a status, a volatile or a substitute: what changes on a side in one turn-step is the foe's doing."""
    return all(int(b[k, _stored(b[k], s, 0) + 20]) == 0 and u32(b[k], s * SIDE + ACTIVE + 16) == 0 and u32(b[k], s * SIDE + ACTIVE + 20) == 0
               for s in range(2))


@functools.lru_cache(maxsize=None)
def _accuracy_states():
    base_b, base_d, base_r, free, _ = _bases()
    pool = [k for k in free if _clean(base_b, k)]
    assert len(pool) >= 16, len(pool)
    rows, tags, take = [], [], 0
    for acc, name in ACCURACY_MOVES.items():
        mid = _move(name)
        assert gamedata.MOVES[mid - 1][3] == acc, (name, acc)
        for a in STAGES:
            for e in STAGES:
                k = pool[take % len(pool)]
                take += 1
                b, d, r = base_b[k].copy(), base_d[k].copy(), int(base_r[k])
                for s in range(2):
                    _all_slots(b, s, mid)
                    _set_bench(b, s, 0)  # nobody to switch to: both sides use the move
                _set_stage(b, 0, 4, a)   # P1 attacks at accuracy a into evasion e ...
                _set_stage(b, 1, 5, e)
                _set_stage(b, 1, 4, e)   # ... and P2 at accuracy e into evasion a
                _set_stage(b, 0, 5, a)
                rows.append((b, d, r))
                tags.append((acc, a, e))
    return rows, tuple(tags)


@functools.lru_cache(maxsize=None)
def _stat_states():
    base_b, base_d, base_r, free, _ = _bases()
    rows, tags, take = [], [], 0
    for eff, mid in sorted(_stage_moves().items()):
        idx, n, on_user = STAGE_EFFECTS[eff]
        for stage in STAGES:
            for stat in STATS:
                k = free[take % len(free)]
                s = take % 2             # the mover: each player in turn
                take += 1
                b, d, r = base_b[k].copy(), base_d[k].copy(), int(base_r[k])
                _all_slots(b, s, mid)
                t = s if on_user else 1 - s
                _set_stage(b, t, idx, stage)
                now = min(max(_scaled(stat, stage), 1), 999)
                for o, v in ((_stored(b, t, 0) + 2 + 2 * idx, stat), (t * SIDE + ACTIVE + 2 + 2 * idx, now)):
                    b[o], b[o + 1] = v & 0xFF, v >> 8
                rows.append((b, d, r))
                tags.append((eff, stage, stat))
    return rows, tuple(tags)


@functools.lru_cache(maxsize=None)
def _cases():
    """Every state under SEEDS choice streams and the oracle's turn-step of each (computed once, read-only); the tags; how many are accuracy cases."""
    acc_rows, acc_tags = _accuracy_states()
    stat_rows, stat_tags = _stat_states()
    rows, tags = acc_rows + stat_rows, acc_tags + stat_tags
    b = np.repeat(np.stack([x[0] for x in rows]), SEEDS, axis=0)
    d = np.repeat(np.stack([x[1] for x in rows]), SEEDS, axis=0)
    r = np.repeat(np.array([x[2] for x in rows], dtype=np.uint8), SEEDS)
    p = np.zeros((len(b), 8), dtype=np.uint8)
    O.LIB.oracle_fast_prng_seed_batch(O.ptr(p), len(p), C.c_uint64(0x31C0FFEE0000))
    ob, od, op = b.copy(), d.copy(), p.copy()
    oout, osteps = O.rollout_batch(ob, od, r, op, max_steps=1, threads=8)
    exp = dict(results=oout, steps=osteps, prng=op, battles=ob, durations=od)
    for a in (b, d, r, p) + tuple(exp.values()):
        a.setflags(write=False)
    return b, d, r, p, exp, tuple(t for t in tags for _ in range(SEEDS)), len(acc_rows) * SEEDS


def _accuracy(acc, a, e):
    x = _scaled(_scaled(acc, a), -e)
    return min(max(x, 1), 255)


def _touched(b, ob, s):
    """Did side s's active Pokemon lose HP or gain a volatile in the turn-step (the states are _clean: only the foe's move does that)?"""
    o = _stored(b, s, 0)
    return u16(ob, o + 18) < u16(b, o + 18) or _vlo(ob, s) & V["CONFUSION"] != 0


def test_the_oracle_accepts_the_cases_and_every_stage_both_lands_and_fails():
    b, d, r, p, exp, tags, n_acc = _cases()
    assert ((exp["results"] & 15) != 4).all() and (exp["steps"] == 1).all()
    assert {t[0] for t in tags[:n_acc]} == set(ACCURACY_MOVES) and {t[0] for t in tags[n_acc:]} == set(STAGE_EFFECTS)
    assert {t[1:] for t in tags[:n_acc]} == {(a, e) for a in STAGES for e in STAGES}
    assert {t[1:] for t in tags[n_acc:]} == {(st, v) for st in STAGES for v in STATS}
    # P1's move into P2, by P1's accuracy stage and by P2's evasion stage: wherever the accuracies of a stage's cases add up to at least
    # eight expected hits (misses), one case of it lands (fails) -- a type immunity looks like a failure here, so hits are counted at half
    for kind in (1, 2):
        landed, failed = set(), set()
        hits, misses = {}, {}
        for k in range(n_acc):
            acc, a, e = tags[k]
            if acc == 76:
                continue
            key = (acc, tags[k][kind])
            chance = _accuracy(acc, a, e)
            chance = 256 if chance == 255 else chance    # 255 is not rolled for
            hits[key] = hits.get(key, 0) + chance / 512
            misses[key] = misses.get(key, 0) + (256 - chance) / 256
            (landed if _touched(b[k], exp["battles"][k], 1) else failed).add(key)
        assert len(hits) == 6 * 13
        assert {key for key, n in hits.items() if n >= 8} <= landed, (kind, sorted(set(hits) - landed))
        assert {key for key, n in misses.items() if n >= 8} <= failed, (kind, sorted(set(misses) - failed))
        assert len(landed) == 6 * 13 and len(failed) >= 6 * 10, (kind, len(landed), len(failed))
    # the stat cases reach the cap, the floor and a stage change in both directions
    stat_now = lambda img, k, t, idx: u16(img[k], t * SIDE + ACTIVE + 2 + 2 * idx)
    seen = set()
    for k in range(n_acc, len(tags)):
        eff, stage, stat = tags[k]
        idx, n, on_user = STAGE_EFFECTS[eff]
        s = ((k - n_acc) // SEEDS) % 2
        t = s if on_user else 1 - s
        before, after = stat_now(b, k, t, idx), stat_now(exp["battles"], k, t, idx)
        if after != before:
            seen.add((eff, "moved"))
            seen.add("cap" if after == 999 else "floor" if after == 1 else "between")
    assert {(eff, "moved") for eff in STAGE_EFFECTS} <= seen and {"cap", "floor", "between"} <= seen, sorted(map(str, seen))


@pytest.fixture
def ctx(gpu_ctx):
    _spread(gpu_ctx, 0)
    try:
        yield gpu_ctx
    finally:
        _spread(gpu_ctx, -1)


@pytest.mark.gpu
def test_one_turn_step_of_every_case_through_the_group_launch(ctx):
    b, d, r, p, exp, tags, _ = _cases()
    got = ctx.rollout_group([(b, d, r, p)], max_steps=1, return_state=True)[0]
    _compare(got, exp, tuple(map(str, tags)), "rollout_group")


@pytest.mark.gpu
def test_one_turn_step_of_every_case_through_rollout(ctx):
    b, d, r, p, exp, tags, _ = _cases()
    got = ctx.rollout(b, d, r, p, max_steps=1, return_state=True)
    _compare(got, exp, tuple(map(str, tags)), "rollout")
