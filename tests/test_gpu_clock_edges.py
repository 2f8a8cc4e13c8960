"""EngineR's turn bookkeeping (before_move, handle_residual, faint / check_faint and on_begin's Heal and Substitute,
oak_amd/csrc/gen1_regs.hpp) against the CPU oracle on the constructed states of tests/clock_cases.py -- the residual's floor of 1 and
its last HP, the 5-bit toxic counter at 15, 16 and 31 with Leech Seed stepping it twice, the capped leech heal, the recovery failure
at 255, 511 and 767 HP lost, Substitute at exactly a quarter, every value of the sleep, confusion, disable, attacking and binding
counters with the duration values beside them (those no game reaches included: there is no rule for them, but the two engines must
still agree), Rest's extended sleep, flinch and recharge, and the locks a full paralysis or a confusion self-hit ends -- byte for byte,
through every kernel that plays a turn: the group launch, rollout, the queue kernel at 17 turn-steps with and without the durations
word (a counter that is one bit too narrow shows in the sixteen turns after), the stepwise update with its 16-byte chance-action key,
where the sleep, confusion, disable, attacking and binding observations live, and the tree step with the key and both players' next
choices (the forced choice under thrash and binding, the recharge's single one).  tests/test_clock_ref.py holds the oracle itself to an
independent restatement of the rules, and says on the oracle's side alone that the cases reach what they are built for.

The launches are small and run with the lane spread off, like tests/test_gpu_damage_edges.py's, whose fixture this file shares."""
import numpy as np
import pytest

import clock_cases as K
from test_gpu_choice_draw import _compare
from test_gpu_damage_edges import _compare_but_durations, _tags, ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def test_one_turn_step_of_every_case_through_the_group_launch(ctx):  # noqa: F811
    b, d, r, p, exp, tags, _ = K.cases()
    got = ctx.rollout_group([(b, d, r, p)], max_steps=1, return_state=True)[0]
    _compare(got, exp, _tags(tags), "rollout_group")


def test_one_turn_step_of_every_case_through_rollout(ctx):  # noqa: F811
    b, d, r, p, exp, tags, _ = K.cases()
    got = ctx.rollout(b, d, r, p, max_steps=1, return_state=True)
    _compare(got, exp, _tags(tags), "rollout")


def test_every_case_through_the_queue_kernel_with_and_without_the_durations_word(ctx):  # noqa: F811
    """17 turn-steps, the smallest cap at which a group launch runs the queue kernel: taking no durations back, lean and not, and once
    taking them back; and one turn-step taking none back."""
    b, d, r, p, one, tags, _ = K.cases()
    exp = K.queue_steps()
    ctx.set_playouts_per_lane(2)
    for lean in (1, 0):
        ctx.set_lean_rollout(lean)
        got = ctx.rollout_group([(b, d, r, p)], max_steps=K.QUEUE_STEPS, return_state=True, return_durations=False)[0]
        assert ctx.last_launch_lean() == bool(lean), lean
        assert "durations" not in got
        _compare_but_durations(got, exp, _tags(tags), ("queue kernel", "lean %d" % lean))
        assert ctx.queue_counters()[63] == 0
    ctx.set_lean_rollout(1)
    got = ctx.rollout_group([(b, d, r, p)], max_steps=K.QUEUE_STEPS, return_state=True)[0]
    assert not ctx.last_launch_lean()
    _compare(got, exp, _tags(tags), "queue kernel, durations taken back")
    got = ctx.rollout_group([(b, d, r, p)], max_steps=1, return_state=True, return_durations=False)[0]
    _compare_but_durations(got, one, _tags(tags), "one turn-step, no durations back")


def test_every_case_through_update_with_the_action_key(ctx):  # noqa: F811
    b, d, r, p, exp, tags, _ = K.cases()
    c1, c2, act, _, _ = K.keyed()
    gb, gd = b.copy(), d.copy()
    gres, gact = ctx.update(gb, c1, c2, gd)
    bad = (gb != exp["battles"]).any(axis=1) | (gres != exp["results"]) | (gd != exp["durations"]).any(axis=1) | (gact != act).any(axis=1)
    assert not bad.any(), (int(bad.sum()), sorted({str(tags[k]) for k in np.where(bad)[0]})[:40])


def test_every_case_through_the_tree_step_with_the_key_and_the_next_choices(ctx):  # noqa: F811
    """oakgpu_tree_step_dev at 39 damage rolls (no clamp) and clamped to one: battle, result, durations, action key and both players'
    next choices against the oracle's."""
    from hipmem import Dev
    b, d, r, _, exp, tags, _ = K.cases()
    c1, c2, act, nxt1, nxt2 = K.keyed()
    want = {39: (exp["battles"], exp["durations"], exp["results"], act, nxt1, nxt2), 1: K.one_roll()}
    n = len(b)
    lib, h = ctx.lib, ctx.handle
    dev = dict(b=Dev(b), d=Dev(d), r=Dev(r), c1=Dev(c1), c2=Dev(c2), act=Dev(np.zeros((n, 16), np.uint8)),
               ch1=Dev(np.zeros((n, 9), np.uint8)), n1=Dev(np.zeros(n, np.uint8)), ch2=Dev(np.zeros((n, 9), np.uint8)), n2=Dev(np.zeros(n, np.uint8)))
    try:
        for rolls in (39, 1):
            dev["b"].put(b)
            dev["d"].put(d)
            dev["r"].put(r)
            assert lib.oakgpu_tree_step_dev(h, dev["b"].p, dev["d"].p, dev["r"].p, dev["c1"].p, dev["c2"].p, n, rolls, dev["act"].p,
                                            dev["ch1"].p, dev["n1"].p, dev["ch2"].p, dev["n2"].p) == 0, rolls
            ctx.synchronize()
            ob, od, ores, oact, o1, o2 = want[rolls]
            bad = ((dev["b"].host() != ob).any(axis=1) | (dev["d"].host() != od).any(axis=1) | (dev["r"].host() != ores) |
                   (dev["act"].host() != oact).any(axis=1))
            forced = 0
            for (ch, cnt), nxt in (((dev["ch1"].host(), dev["n1"].host()), o1), ((dev["ch2"].host(), dev["n2"].host()), o2)):
                for i, o in enumerate(nxt):
                    if o is not None:
                        bad[i] |= cnt[i] != len(o) or (ch[i, :len(o)] != o).any()
                        forced += len(o) == 1
            assert forced >= 1000, forced
            assert not bad.any(), (rolls, int(bad.sum()), sorted({str(tags[k]) for k in np.where(bad)[0]})[:40])
    finally:
        for x in dev.values():
            x.free()
