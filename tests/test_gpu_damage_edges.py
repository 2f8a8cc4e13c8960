"""EngineR's damage path (check_crit, calc_damage with fast_div24, adjust_damage, randomize_damage, apply_damage and run_move's
fixed-damage branch, oak_amd/csrc/gen1_regs.hpp) against the CPU oracle at its arithmetic edges: the constructed states of
tests/damage_cases.py -- the byte boundary of the stat scaling and its wrap to 1 under a screen, the cap of 997, levels 1 to 255, every
cell of the type chart with its two truncations, damage of 0 and 1, Explosion's halved defence, the fixed-damage moves, the confusion
self-hit and a critical hit under Transform -- byte for byte, through every kernel that plays a turn: the group launch with and without
the durations word (the lean instantiation), rollout, the stepwise update with its chance-action key, and the tree step under every
damage-roll clamp.  tests/test_damage_ref.py holds the oracle itself to an independent restatement of the arithmetic, and says on the
oracle's side alone that the cases reach what they are built for.

The Transform states are made by hand (the volatile, the copied identity, stats, species, types and moves as a Transform leaves
them); the oracle accepts them.  The launches are small and run with the lane spread off, like tests/test_gpu_choice_draw.py's."""
import numpy as np
import pytest

import damage_cases as D
from test_gpu_choice_draw import _compare, _spread
from test_gpu_lean_rollout import CARRY_DEFAULT, LEAN_DEFAULT

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx(gpu_ctx):
    """The session's context with no lane spread; every setter back to its default afterwards."""
    _spread(gpu_ctx, 0)
    try:
        yield gpu_ctx
    finally:
        _spread(gpu_ctx, -1)
        gpu_ctx.set_playouts_per_lane(2)
        gpu_ctx.set_move_carry(CARRY_DEFAULT)
        gpu_ctx.set_lean_rollout(LEAN_DEFAULT)


def _tags(tags):
    return tuple(map(str, tags))


def _compare_but_durations(got, exp, tags, what):
    bad = np.zeros(len(tags), dtype=bool)
    for key in ("results", "steps", "prng", "battles"):
        ne = got[key] != exp[key]
        bad |= ne if ne.ndim == 1 else ne.any(axis=1)
    assert not bad.any(), (what, int(bad.sum()), sorted({tags[k] for k in np.where(bad)[0]}))


def test_one_turn_step_of_every_case_through_the_group_launch(ctx):
    b, d, r, p, exp, tags, _, _ = D.cases()
    got = ctx.rollout_group([(b, d, r, p)], max_steps=1, return_state=True)[0]
    _compare(got, exp, _tags(tags), "rollout_group")


def test_every_case_through_the_queue_kernel_with_and_without_the_durations_word(ctx):
    """A group launch capped at 16 turn-steps or fewer never runs the queue kernel, so none of the launches above reaches the lean
    instantiation (the one that keeps no durations word): it takes a cap of 17.  Every case, then, for 17 turn-steps -- the first one at
    the edge the case is built for, the rest with the same stats until somebody faints -- taking no durations back, lean and not, and
    once taking them back."""
    b, d, r, p, _, tags, _, _ = D.cases()
    exp = D.queue_steps()
    ctx.set_playouts_per_lane(2)
    for lean in (1, 0):
        ctx.set_lean_rollout(lean)
        got = ctx.rollout_group([(b, d, r, p)], max_steps=D.QUEUE_STEPS, return_state=True, return_durations=False)[0]
        assert ctx.last_launch_lean() == bool(lean), lean
        assert "durations" not in got
        _compare_but_durations(got, exp, _tags(tags), ("queue kernel", "lean %d" % lean))
        assert ctx.queue_counters()[63] == 0
    ctx.set_lean_rollout(1)
    got = ctx.rollout_group([(b, d, r, p)], max_steps=D.QUEUE_STEPS, return_state=True)[0]
    assert not ctx.last_launch_lean()
    _compare(got, exp, _tags(tags), "queue kernel, durations taken back")
    # and one turn-step taking no durations back: the staged kernel without a durations_out
    got = ctx.rollout_group([(b, d, r, p)], max_steps=1, return_state=True, return_durations=False)[0]
    _compare_but_durations(got, D.cases()[4], _tags(tags), "one turn-step, no durations back")


def test_one_turn_step_of_every_case_through_rollout(ctx):
    b, d, r, p, exp, tags, _, _ = D.cases()
    got = ctx.rollout(b, d, r, p, max_steps=1, return_state=True)
    _compare(got, exp, _tags(tags), "rollout")


def test_the_plain_cases_through_update_with_the_action_key(ctx):
    """The rollout paths never show the 16-byte chance-action key (critical hit, hit, damage roll, Psywave): the stepwise update does."""
    b, d, r, p, exp, tags, _, _ = D.cases()
    c1, c2, act = D.keyed()
    lanes = D.plain_subset()
    gb, gd = b[lanes].copy(), d[lanes].copy()
    gres, gact = ctx.update(gb, c1[lanes], c2[lanes], gd)
    bad = ((gb != exp["battles"][lanes]).any(axis=1) | (gres != exp["results"][lanes]) | (gd != exp["durations"][lanes]).any(axis=1) |
           (gact != act[lanes]).any(axis=1))
    assert not bad.any(), (int(bad.sum()), sorted({str(tags[k]) for k in lanes[bad]}))


def test_the_damage_roll_clamps_through_the_tree_step(ctx):
    """256 plain cases through oakgpu_tree_step_dev under every clamp it takes -- 1, 2, 3, 20 and 39 (none) damage rolls; every other
    count from 1 to 39 is refused before anything is launched -- against the oracle stepped with the override bytes of that clamp:
    battle, result, durations, action key and both players' next choices."""
    from hipmem import Dev
    b, d, r, _, _, tags, _, _ = D.cases()
    c1, c2, _ = D.keyed()
    lanes, want = D.roll_cases()
    n = len(lanes)
    assert set(want) == set(D.ROLLS)
    lib, h = ctx.lib, ctx.handle
    dev = dict(b=Dev(b[lanes]), d=Dev(d[lanes]), r=Dev(r[lanes]), c1=Dev(c1[lanes]), c2=Dev(c2[lanes]), act=Dev(np.zeros((n, 16), np.uint8)),
               ch1=Dev(np.zeros((n, 9), np.uint8)), n1=Dev(np.zeros(n, np.uint8)), ch2=Dev(np.zeros((n, 9), np.uint8)), n2=Dev(np.zeros(n, np.uint8)))
    step = lambda rolls: lib.oakgpu_tree_step_dev(h, dev["b"].p, dev["d"].p, dev["r"].p, dev["c1"].p, dev["c2"].p, n, rolls, dev["act"].p,
                                                  dev["ch1"].p, dev["n1"].p, dev["ch2"].p, dev["n2"].p)
    try:
        for rolls in range(1, 40):
            if rolls not in D.ROLLS:
                assert step(rolls) != 0, rolls
                continue
            dev["b"].put(b[lanes])
            dev["d"].put(d[lanes])
            dev["r"].put(r[lanes])
            assert step(rolls) == 0, rolls
            ctx.synchronize()
            ob, od, ores, oact, nxt1, nxt2 = want[rolls]
            bad = ((dev["b"].host() != ob).any(axis=1) | (dev["d"].host() != od).any(axis=1) | (dev["r"].host() != ores) |
                   (dev["act"].host() != oact).any(axis=1))
            for (ch, cnt), nxt in (((dev["ch1"].host(), dev["n1"].host()), nxt1), ((dev["ch2"].host(), dev["n2"].host()), nxt2)):
                for i, o in enumerate(nxt):
                    if o is not None:
                        bad[i] |= cnt[i] != len(o) or (ch[i, :len(o)] != o).any()
            assert not bad.any(), (rolls, int(bad.sum()), sorted({str(tags[k]) for k in lanes[bad]}))
    finally:
        for x in dev.values():
            x.free()


def test_two_turn_steps_of_the_cap_fixed_and_explode_cases(ctx):
    """The turn after: a switch request behind a faint, a broken substitute, the recharge, and Counter doubling the last_damage that the
    first turn-step left."""
    b, d, r, p, exp, tags = D.two_steps()
    got = ctx.rollout_group([(b, d, r, p)], max_steps=2, return_state=True)[0]
    _compare(got, exp, _tags(tags), "rollout_group, two turn-steps")
