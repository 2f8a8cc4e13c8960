"""k_rollout_queue writes a lane's image -- finished, donated or parked -- from copies of the sides taken by player, and leaves the
engine's own frame where the turn ended; and a dry bulk wave may go on carrying second moves (oakgpu_set_move_carry_dry).  Per playout
nothing changes, so every output byte must equal the CPU oracle's.  What can go wrong: an image stored from the wrong frame (sides
exchanged, or the actives' write-back to the party going to the other player), a lane in mid-turn that is parked or retired, a wave
that suspends or leaves with a pending action.  Small launches, lane spread off (a spread launch never carries).

Preconditions are checked on the ORACLE's playouts alone.  The oracle stores by player and keeps no frame, so "ends in a flipped frame"
cannot be read off its outputs; what can: after turn 0 (both leads out, frame as loaded) the first real turn orders the sides by the
actives' speed, and the group holds playouts with either side the faster one -- the frame then changes with every action and every
second-mover-first turn, ~100 turns per playout, so both frames occur among a few hundred final images beyond any doubt."""
import functools
import os
import re

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "include", "oakgpu.h")).read()
CARRY_DEFAULT = int(re.search(r"#define\s+OAKGPU_MOVE_CARRY_DEFAULT\s+(\d+)", _HDR).group(1))
DRY_DEFAULT = int(re.search(r"#define\s+OAKGPU_MOVE_CARRY_DRY_DEFAULT\s+(\d+)", _HDR).group(1))
KEYS = ("results", "steps", "values", "prng", "battles", "durations")


@functools.lru_cache(maxsize=None)
def _batches(sizes, seed0):
    out = tuple(O.make_random_ou_batch(n, seed0=seed0 + 7919 * k) for k, n in enumerate(sizes))
    for batch in out:
        for a in batch:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(sizes, seed0, max_steps):
    """The oracle's outputs, once per (inputs, cap), shared by every schedule setting."""
    exp = []
    for b, d, p, r in _batches(sizes, seed0):
        ob, od, op = b.copy(), d.copy(), p.copy()
        oout, osteps = O.rollout_batch(ob, od, r, op, max_steps=max_steps, threads=8)
        t = oout & 15
        exp.append(dict(results=oout, steps=osteps, values=np.where(t == 1, 1.0, np.where(t == 2, 0.0, 0.5)).astype(np.float32),
                        prng=op, battles=ob, durations=od))
    return exp


def _run(ctx, sizes, seed0, max_steps):
    return ctx.rollout_group([(b, d, r, p) for b, d, p, r in _batches(sizes, seed0)], max_steps=max_steps, return_state=True)


def _same(got, exp, what):
    for k, (g, e) in enumerate(zip(got, exp)):
        for key in KEYS:
            bad = g[key] != e[key]
            assert not bad.any(), (what, "batch %d" % k, key, int(bad.reshape(len(bad), -1).any(axis=1).sum()))


def _spread(ctx, lanes):
    from oak_amd import _lib
    _lib.check(ctx.lib.oakgpu_set_spread(ctx.handle, lanes))


@pytest.fixture
def ctx(gpu_ctx):
    """The session's context at two playouts per lane and no lane spread; every schedule setting back to its default afterwards."""
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


FRAMES = ((192, 192), 0x18F00000)


def _active_speeds(battles):
    """(P1's, P2's) active speed of 384-byte images: the high half of the second active dword of each side."""
    w = np.ascontiguousarray(battles).view(np.uint32).reshape(len(battles), 96)
    return w[:, 37] >> 16, w[:, 83] >> 16


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", (1, 2, 7, 17, 1000))
def test_finished_images_in_either_frame(ctx, max_steps):
    """2 batches x 192 playouts with both image outputs given, caps 1, 2, 7 (the short-launch kernels, whose store goes through the
    same two-sided store), 17 (the smallest the queue kernel runs: every lane stops where its 17th turn left the frame) and 1,000."""
    after_leads = _oracle(*FRAMES, 1)
    s1, s2 = (np.concatenate(x) for x in zip(*(_active_speeds(e["battles"]) for e in after_leads)))
    assert (s1 > s2).sum() > 20 and (s1 < s2).sum() > 20, "the first real turn does not put the sides in either order"
    exp = _oracle(*FRAMES, max_steps)
    steps = np.concatenate([e["steps"] for e in exp])
    assert (steps == max_steps).all() if max_steps < 1000 else steps.max() < 1000  # stopped by the cap / ended by the game itself
    for carry, dry in ((CARRY_DEFAULT, DRY_DEFAULT), (0, 0), (64, 1)):
        ctx.set_move_carry(carry)
        ctx.set_move_carry_dry(dry)
        _same(_run(ctx, *FRAMES, max_steps), exp, (max_steps, carry, dry))
    assert ctx.queue_counters()[63] == 0


DONATE = ((512,), 0x18F10000)


@pytest.mark.gpu
@pytest.mark.parametrize("dry", (0, 8))
def test_donated_images(ctx, dry):
    """Migration forced on, a playout is donated once it has run 4 turn-steps, one adopter: every image the adopter loads was
    written by a bulk wave from whichever frame the playout stood in."""
    exp = _oracle(*DONATE, 1000)
    assert (exp[0]["steps"] > 4).sum() > 256, "too few of the oracle's playouts outlast long_steps"
    ctx.set_migration(2, 4, 1)
    ctx.set_move_carry_dry(dry)
    _same(_run(ctx, *DONATE, 1000), exp, ("donated", dry))
    c = ctx.queue_counters()
    assert c[63] == 0, ("bounded wait ran out", int(c[63]))
    assert c[40] > 0 and c[40] == c[41], ("donations / adoptions", int(c[40]), int(c[41]))


PARK = ((1024,), 0x18F20000)


@pytest.mark.gpu
@pytest.mark.parametrize("dry", (0, 8, 64))
def test_parked_images(ctx, dry):
    """Three regrouping rounds, a dry wave with fewer than 48 live lanes parks them, each round a half of the waves: a parked image
    is a completed turn's -- with dry carry on, the wave flushes before it suspends."""
    exp = _oracle(*PARK, 1000)
    steps = exp[0]["steps"]
    assert steps.max() > 4 * np.median(steps), "no long tail: nothing would be left to park"
    ctx.set_migration(0)
    ctx.set_regroup(3, 48, 2)
    ctx.set_move_carry_dry(dry)
    _same(_run(ctx, *PARK, 1000), exp, ("parked", dry))
    c = ctx.queue_counters()
    assert c[1] > 0, "no lane was parked"
    assert c[63] == 0


CARRY = ((2048,), 0x18F30000)
PAIRS = [(c, d) for c in (0, 1, 32, 64) for d in (0, 1, 8, 64)]


_CARRY_OFF = {}  # standstill skip on / off -> the launch's outputs at carry 0 / 0, taken once


@pytest.mark.gpu
@pytest.mark.parametrize("carry,dry", PAIRS)
def test_carrying_in_bulk_and_dry_waves(ctx, carry, dry):
    """2,048 playouts at 2 per lane: 16 full waves whose queue runs dry after one refill each, with lanes in mid-turn wherever the
    wave carried.  Every pair of thresholds, standstill skip on and off: identical to carry 0 / 0 and to the oracle."""
    exp = _oracle(*CARRY, 1000)
    steps = exp[0]["steps"]
    # the waves outlive their queue: the longest playouts run on for many turns after the others' lanes have nothing left to take
    assert steps.max() > 4 * np.median(steps) and (steps > 2 * np.median(steps)).sum() >= 16
    for skip in (True, False):
        ctx.set_standstill_skip(skip)
        if skip not in _CARRY_OFF:
            ctx.set_move_carry(0)
            ctx.set_move_carry_dry(0)
            _CARRY_OFF[skip] = _run(ctx, *CARRY, 1000)
        ref = _CARRY_OFF[skip]
        ctx.set_move_carry(carry)
        ctx.set_move_carry_dry(dry)
        got = _run(ctx, *CARRY, 1000)
        _same(got, ref, (carry, dry, skip, "against carry 0 / 0"))
        _same(got, exp, (carry, dry, skip, "against the oracle"))
        assert ctx.queue_counters()[63] == 0


@pytest.mark.gpu
def test_the_dry_setter_checks_its_range(ctx):
    lib = ctx.lib
    for below in (-1, 65, 1 << 20, -(1 << 31)):
        assert lib.oakgpu_set_move_carry_dry(ctx.handle, below) != 0, below
        assert b"oakgpu_set_move_carry_dry" in lib.oakgpu_last_error()
    for below in (0, 1, 64, DRY_DEFAULT):
        assert lib.oakgpu_set_move_carry_dry(ctx.handle, below) == 0, below
