"""k_rollout_queue's lean instantiation (oakgpu_set_lean_rollout): a group launch none of whose batches takes durations back runs an
engine that keeps no chance-durations word -- none loaded but for the prep of a fresh playout, none parked with a donated or
suspended playout, none written.  Per playout nothing else may change: results, step counts, values, the advanced prng and, where
asked for, the final 384-byte battles are byte for byte the CPU oracle's, with the lean kernel and with the one that keeps durations.
What can go wrong: a transition that did read the word after all, a prep that reads a stale or missing word, a parked image resumed
with another playout's durations, a standstill skipped that the battle alone does not prove.

The inputs are mid-game states with non-zero durations (tests/lean_ref.py): a fresh battle's are all zero and cannot tell a stale load
from none.  Small launches, two playouts per lane, lane spread off, as tests/test_gpu_queue_frames.py."""
import os
import re

import numpy as np
import pytest

import inert_ref as R
import lean_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "include", "oakgpu.h")).read()
_default = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, _HDR).group(1))
CARRY_DEFAULT, DRY_DEFAULT, LEAN_DEFAULT = _default("OAKGPU_MOVE_CARRY_DEFAULT"), _default("OAKGPU_MOVE_CARRY_DRY_DEFAULT"), _default("OAKGPU_LEAN_ROLLOUT_DEFAULT")
VALUE_KEYS = ("results", "steps", "values", "prng")
FFWD = 44  # OAKGPU_CTL_FAST_FORWARDED


def _spread(ctx, lanes):
    from oak_amd import _lib
    _lib.check(ctx.lib.oakgpu_set_spread(ctx.handle, lanes))


@pytest.fixture
def ctx(gpu_ctx):
    """The session's context at two playouts per lane and no lane spread; every setter back to its default afterwards."""
    gpu_ctx.set_playouts_per_lane(2)
    _spread(gpu_ctx, 0)
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_playouts_per_lane(2)
        _spread(gpu_ctx, -1)
        gpu_ctx.set_move_carry(CARRY_DEFAULT)
        gpu_ctx.set_move_carry_dry(DRY_DEFAULT)
        gpu_ctx.set_regroup()
        gpu_ctx.set_migration(1, 300, 0)
        gpu_ctx.set_migration_window(48)
        gpu_ctx.set_standstill_skip(True)
        gpu_ctx.set_lean_rollout(LEAN_DEFAULT)


def _inputs(sizes, seed0):
    """One mid-game batch per size; on the oracle's states alone: durations are live in every batch."""
    out = [L.midgame(n, seed0 + 7919 * k) for k, n in enumerate(sizes)]
    for (b, d, p, r), n in zip(out, sizes):
        lanes, attacking, binding = L.census(d, r)
        assert lanes >= n // 16 and attacking >= 1, ("the inputs carry too few live durations", n, lanes, attacking, binding)
    return out


def _same(got, exp, keys, what):
    for k, (g, e) in enumerate(zip(got, exp)):
        for key in keys:
            bad = g[key] != e[key]
            assert not bad.any(), (what, "batch %d" % k, key, int(bad.reshape(len(bad), -1).any(axis=1).sum()))


def _run(ctx, batches, lean, max_steps=1000, prep=False, state=True):
    """One group launch that takes no durations back, with the lean kernel asked for or not; says which kernel ran."""
    ctx.set_lean_rollout(lean)
    got = ctx.rollout_group([(b, d, r, p) for b, d, p, r in batches], max_steps=max_steps, prep=prep, return_state=state, return_durations=False)
    assert ctx.last_launch_lean() == bool(lean), ("asked for lean = %d" % lean, ctx.last_launch_lean())
    return got


def _both_equal_the_oracle(ctx, batches, exp, what, max_steps=1000, prep=False, state=True):
    keys = VALUE_KEYS + (("battles",) if state else ())
    for lean in (1, 0):
        _same(_run(ctx, batches, lean, max_steps, prep, state), exp, keys, (what, "lean %d" % lean))
        assert ctx.queue_counters()[63] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", (17, 1000))
def test_two_batches_with_the_final_battles(ctx, max_steps):
    """2 x 192 playouts, the final battles taken back and no durations: cap 17 (the smallest the queue kernel runs) and 1,000."""
    batches = _inputs((192, 192), 0x32A00000)
    exp = [L.play(b, d, p, r, max_steps) for b, d, p, r in batches]
    _both_equal_the_oracle(ctx, batches, exp, max_steps, max_steps)
    _both_equal_the_oracle(ctx, batches, exp, (max_steps, "values only"), max_steps, state=False)


@pytest.mark.gpu
def test_donated_and_adopted_without_a_parked_durations_word(ctx):
    """Migration forced on, a playout is donated after 4 turn-steps, one adopter: the lean kernel writes and reads the battle image alone."""
    batches = _inputs((512,), 0x32A10000)
    exp = [L.play(*batches[0])]
    assert (exp[0]["steps"] > 4).sum() > 128, "too few of the oracle's playouts outlast long_steps"
    ctx.set_migration(2, 4, 1)
    for lean in (1, 0):
        _same(_run(ctx, batches, lean), exp, VALUE_KEYS + ("battles",), ("donated", lean))
        c = ctx.queue_counters()
        assert c[63] == 0, ("bounded wait ran out", int(c[63]))
        assert c[40] > 0 and c[40] == c[41], ("donations / adoptions", lean, int(c[40]), int(c[41]))


@pytest.mark.gpu
def test_parked_and_resumed_across_rounds(ctx):
    """Three regrouping rounds, a dry wave with fewer than 48 live lanes parks them: the later rounds run the round-0 instantiation."""
    batches = _inputs((1024,), 0x32A20000)
    exp = [L.play(*batches[0])]
    steps = exp[0]["steps"]
    assert steps.max() > 4 * max(np.median(steps), 1), "no long tail: nothing would be left to park"
    ctx.set_migration(0)
    ctx.set_regroup(3, 48, 2)
    for lean in (1, 0):
        _same(_run(ctx, batches, lean), exp, VALUE_KEYS + ("battles",), ("parked", lean))
        c = ctx.queue_counters()
        assert c[1] > 0, "no lane was parked"
        assert c[63] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("carry,dry", ((0, 0), (CARRY_DEFAULT, DRY_DEFAULT), (64, 1)))
def test_move_carry(ctx, carry, dry):
    """2,048 playouts: 16 full waves, lanes in mid-turn wherever the wave carried."""
    batches = _inputs((2048,), 0x32A30000)
    exp = [L.play(*batches[0])]
    ctx.set_move_carry(carry)
    ctx.set_move_carry_dry(dry)
    _both_equal_the_oracle(ctx, batches, exp, ("carry", carry, dry))


@pytest.mark.gpu
def test_prep_reads_the_input_durations_once(ctx):
    """prep = 1 at 512 playouts: the lean kernel loads a fresh playout's durations for its hidden-variable draw and drops them."""
    batches = _inputs((512,), 0x32A40000)
    b, d, p, r = batches[0]
    exp = [L.play(b, d, p, r, prep=True)]
    zeroed = L.play(b, np.zeros_like(d), p, r, prep=True)
    assert any((exp[0][key] != zeroed[key]).any() for key in VALUE_KEYS), "the oracle's prep does not depend on these durations"
    lean, full = _run(ctx, batches, 1, prep=True), _run(ctx, batches, 0, prep=True)
    _same(lean, full, VALUE_KEYS + ("battles",), "prep: lean against full")
    _same(lean, exp, VALUE_KEYS + ("battles",), "prep: lean against the oracle")
    assert ctx.queue_counters()[63] == 0


@pytest.mark.gpu
def test_a_batch_that_takes_durations_back_runs_the_full_kernel(ctx):
    """Two batches, the second with a durations_out: the whole group runs the kernel that keeps durations, and they are the oracle's."""
    batches = _inputs((192, 192), 0x32A50000)
    exp = [L.play(b, d, p, r) for b, d, p, r in batches]
    ctx.set_lean_rollout(1)
    got = ctx.rollout_group([(b, d, r, p) for b, d, p, r in batches], return_state=True, return_durations=(False, True))
    assert not ctx.last_launch_lean()
    _same(got, exp, VALUE_KEYS + ("battles",), "mixed group")
    assert "durations" not in got[0] and (got[1]["durations"] == exp[1]["durations"]).all()
    assert (exp[1]["durations"] != 0).any()


def _stalemates():
    """The accepted stalemate states of tests/test_gpu_inert_standstill.py, each side given a live duration the battle does not show:
    side 1 an attacking count, side 2 a binding count."""
    import test_gpu_inert_standstill as T
    b, d, p, res, _, _ = R.harvest()
    acc = T._accepted(b, d, res)
    assert acc.sum() >= 100
    b, d, p, res = (np.ascontiguousarray(x[acc]) for x in (b, d, p, res))
    w = d.view(np.uint32).reshape(-1, 2)
    w[:, 0] |= np.uint32(1 << 25)
    w[:, 1] |= np.uint32(1 << 28)
    return b, d, p, res


@pytest.mark.gpu
@pytest.mark.parametrize("cap", (300, 1000))
def test_standstill_skip_without_durations(ctx, cap):
    """With durations kept, a skipped stalemate must leave them exact, so a live attacking or binding count refuses the skip; without
    them the battle alone decides.  Either way, skip on or off: the oracle's outputs, which plays every turn."""
    b, d, p, res = _stalemates()
    exp = [L.play(b, d, p, res, cap)]
    ffwd = {}
    for skip in (True, False):
        ctx.set_standstill_skip(skip)
        for lean in (1, 0):
            _same(_run(ctx, [(b, d, p, res)], lean, cap, state=False), exp, VALUE_KEYS, (cap, skip, lean))
            c = ctx.queue_counters()
            assert c[63] == 0
            ffwd[skip, lean] = int(c[FFWD])
    print("fast-forwarded: lean %d, full %d of %d" % (ffwd[True, 1], ffwd[True, 0], len(b)))
    assert ffwd[True, 1] >= ffwd[True, 0]
    assert ffwd[False, 1] == 0 and ffwd[False, 0] == 0
