"""k_rollout_queue's move carry (oakgpu_set_move_carry): a lane's second action of a turn may wait for the wave's next pass through
the action code.  Per playout nothing changes, so every output byte must equal the CPU oracle's at every threshold -- and what can
go wrong is a lane in mid-turn meeting a refill, a step cap, an image store, a donation, a suspend or its wave's exit.  A few dozen
waves whose lanes are refilled about four times each meet all of them.

The small launches run with the lane spread off (oakgpu_set_spread 0): a launch spread over part of its lanes never carries."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = int(re.search(r"#define\s+OAKGPU_MOVE_CARRY_DEFAULT\s+(\d+)", open(os.path.join(ROOT, "include", "oakgpu.h")).read()).group(1))
CARRY = sorted({0, 1, 16, 64, DEFAULT})
SIZES = (1500, 64, 2000)
KEYS = ("results", "steps", "values", "prng", "battles", "durations")


@functools.lru_cache(maxsize=None)
def _group():
    out = tuple(O.make_random_ou_batch(n, seed0=0x16CA0000 + 7919 * k) for k, n in enumerate(SIZES))
    for batch in out:
        for a in batch:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(max_steps, prep):
    """The oracle's outputs of the group, computed once per (cap, prep) and shared by every threshold."""
    exp = []
    for b, d, p, r in _group():
        ob, od, op = b.copy(), d.copy(), p.copy()
        oout, osteps = O.rollout_batch(ob, od, r, op, max_steps=max_steps, prep=prep, threads=8)
        t = oout & 15
        exp.append(dict(results=oout, steps=osteps, values=np.where(t == 1, 1.0, np.where(t == 2, 0.0, 0.5)).astype(np.float32),
                        prng=op, battles=ob, durations=od))
    return exp


def _spread(ctx, lanes):
    from oak_amd import _lib
    _lib.check(ctx.lib.oakgpu_set_spread(ctx.handle, lanes))


@pytest.fixture
def ctx(gpu_ctx):
    """The session's context with four playouts per lane and no lane spread; every schedule setting back to its default afterwards."""
    gpu_ctx.set_playouts_per_lane(4)
    _spread(gpu_ctx, 0)
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_playouts_per_lane(2)
        _spread(gpu_ctx, -1)
        gpu_ctx.set_move_carry(DEFAULT)
        gpu_ctx.set_regroup()
        gpu_ctx.set_migration(1, 300, 0)
        gpu_ctx.set_migration_window(48)
        gpu_ctx.set_standstill_skip(True)
        from oak_amd import _lib
        _lib.check(gpu_ctx.lib.oakgpu_set_tail_pack(gpu_ctx.handle, 0, 0, 0))


def _check_group(ctx, max_steps, prep, what, return_state=True):
    got = ctx.rollout_group([(b, d, r, p) for b, d, p, r in _group()], max_steps=max_steps, prep=prep, return_state=return_state)
    for k, (g, e) in enumerate(zip(got, _oracle(max_steps, prep))):
        for key in KEYS if return_state else KEYS[:4]:
            bad = g[key] != e[key]
            assert not bad.any(), (what, "batch %d" % k, key, int(bad.reshape(len(bad), -1).any(axis=1).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("below", CARRY)
def test_every_output_byte_equals_the_oracle_at_every_cap(ctx, below):
    """Caps 1, 2, 3 and 7 (and 17, 40: the smallest the queue kernel itself runs), the full 1,000, root prep, and with and without the
    final images: a cap is met at a turn's end whether or not the turn's second move was carried, and the final image is a
    completed turn's."""
    ctx.set_move_carry(below)
    for max_steps, prep in ((1000, False), (1000, True), (1, False), (2, False), (3, False), (7, False), (17, False), (40, True)):
        _check_group(ctx, max_steps, prep, (below, max_steps, prep))
    _check_group(ctx, 1000, False, (below, "no images"), return_state=False)
    assert ctx.queue_counters()[63] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("below", CARRY)
def test_donations_happen_while_bulk_waves_carry(ctx, below):
    """Migration forced on, a low step threshold, two adopters: a donated playout's image belongs to a completed turn."""
    ctx.set_move_carry(below)
    for long_steps, window in ((20, 0), (999, 3)):
        ctx.set_migration(2, long_steps, 2)
        ctx.set_migration_window(window)
        for prep in (False, True):
            _check_group(ctx, 1000, prep, (below, long_steps, window, prep))
            c = ctx.queue_counters()
            assert c[63] == 0, ("bounded wait ran out", int(c[63]))
            assert c[40] > 0 and c[40] == c[41], ("donations / adoptions", int(c[40]), int(c[41]))


@pytest.mark.gpu
@pytest.mark.parametrize("below", CARRY)
def test_regrouping_rounds_suspend_and_resume_at_turn_boundaries(ctx, below):
    ctx.set_move_carry(below)
    ctx.set_migration(0)
    for rounds, suspend_below, shrink in ((4, 32, 3), (2, 64, 2), (3, 1, 1)):
        ctx.set_regroup(rounds, suspend_below, shrink)
        for max_steps, prep in ((1000, False), (40, True)):
            _check_group(ctx, max_steps, prep, (below, rounds, suspend_below, shrink, max_steps, prep))


def _device_batch(ctx, n, seed):
    """n random OU playouts made on the device: the buffers of one oakgpu_rollout_dev call (inputs are kept, outputs apart)."""
    from hipmem import Dev
    from oak_amd import _lib
    ctx.ensure_ou_pools()
    z = lambda *s, dt=np.uint8: np.zeros(s, dtype=dt)
    dev = {"b": Dev(z(n, 384), fill=0), "d": Dev(z(n, 8), fill=0), "p0": Dev(z(n, 8), fill=0), "r": Dev(z(n), fill=0), "p": Dev(z(n, 8), fill=0),
           "ro": Dev(z(n), fill=0), "st": Dev(z(n, dt=np.uint32), fill=0), "va": Dev(z(n, dt=np.float32), fill=0),
           "bo": Dev(z(n, 384), fill=0), "do": Dev(z(n, 8), fill=0)}
    _lib.check(ctx.lib.oakgpu_random_ou_battles_dev(ctx.handle, C.c_uint64(seed), n, dev["b"].p, dev["d"].p, dev["p0"].p, dev["r"].p))
    ctx.synchronize()
    return dev


def _run_device_batch(ctx, dev, n, max_steps=1000):
    from hipmem import hip
    from oak_amd import _lib
    assert hip().hipMemcpy(dev["p"].p, dev["p0"].p, n * 8, 3) == 0       # the choice streams advance in place: start from the same ones
    _lib.check(ctx.lib.oakgpu_rollout_dev(ctx.handle, dev["b"].p, dev["d"].p, dev["r"].p, dev["p"].p, n, max_steps, 0, dev["ro"].p, dev["st"].p,
                                          dev["va"].p, dev["bo"].p, dev["do"].p))
    ctx.synchronize()
    return {k: dev[k].host() for k in ("ro", "st", "va", "p", "bo", "do")}


@pytest.mark.gpu
def test_tail_pack_of_a_saturating_launch(ctx):
    """The tail pack applies to launches that fill the device: 2 playouts per lane on every resident wave.  Dry waves park their
    last lanes and a follow-up dispatch finishes them, a few to a wave; carried or not, byte for byte the same (no oracle run)."""
    from oak_amd import _lib
    n = 2 * 64 * 4096 + 1000
    ctx.set_playouts_per_lane(2)
    dev = _device_batch(ctx, n, 0x16CB00000000)
    try:
        _lib.check(ctx.lib.oakgpu_set_tail_pack(ctx.handle, 32, 0, 8))
        ctx.set_move_carry(0)
        ref = _run_device_batch(ctx, dev, n)
        assert ctx.queue_counters()[1] > 0, "no lane was parked: the launch did not take the tail pack"
        for below in [c for c in CARRY if c]:
            ctx.set_move_carry(below)
            got = _run_device_batch(ctx, dev, n)
            assert ctx.queue_counters()[63] == 0
            for key in ref:
                assert np.array_equal(got[key], ref[key]), (below, key)
    finally:
        for x in dev.values():
            x.free()


@pytest.mark.gpu
@pytest.mark.parametrize("below", CARRY)
def test_standstill_skip_on_and_off_on_the_harvested_long_playouts(ctx, below):
    """A lane in mid-turn never evaluates the standstill predicate and is never fast-forwarded."""
    import inert_ref as R
    from test_gpu_inert_standstill import FFWD, _both, _same
    b, d, p, res, _, _ = R.harvest()
    ctx.set_playouts_per_lane(2)
    ctx.set_move_carry(below)
    got, exp = _both(ctx, b, d, p, res, 700)
    c = ctx.queue_counters()
    _same(got, exp, (below, "skip on"))
    assert c[FFWD] > 100 and c[63] == 0
    ctx.set_standstill_skip(False)
    got = ctx.rollout(b, d, res, p, max_steps=700, return_state=True)
    _same(got, exp, (below, "skip off"))
    assert ctx.queue_counters()[FFWD] == 0


@pytest.mark.gpu
def test_two_contexts_with_different_thresholds_launch_concurrently(ctx):
    from hipmem import Dev
    from oak_amd import _lib
    from oak_amd.engine import Context
    nb, n = 2, 10000
    other = Context(0)
    runs = []
    try:
        for k, (c, below) in enumerate(((ctx, 64), (other, 16 if DEFAULT == 0 else 0))):
            c.set_playouts_per_lane(4)
            _spread(c, 0)
            c.set_move_carry(below)
            c.set_migration(2, 60, 4)
            b, d, p, r = O.make_random_ou_batch(nb * n, seed0=0x16CC0000 + k * nb * n)
            dev = {"b": Dev(b), "d": Dev(d), "p": Dev(p), "r": Dev(r), "ro": Dev(r, fill=0), "st": Dev(np.zeros(nb * n, dtype=np.uint32)),
                   "va": Dev(np.zeros(nb * n, dtype=np.float32)), "bo": Dev(b, fill=0), "do": Dev(d, fill=0)}
            batches = (_lib.RolloutBatch * nb)()
            for j in range(nb):
                at = lambda key, stride: C.c_void_p(dev[key].p.value + j * n * stride)
                batches[j] = _lib.RolloutBatch(at("b", 384), at("d", 8), at("r", 1), at("p", 8), n, at("ro", 1), at("st", 4), at("va", 4), at("bo", 384), at("do", 8))
            runs.append((c, dev, batches, (b, d, p, r)))
        for c, dev, batches, _ in runs:            # both launches in flight together
            _lib.check(c.lib.oakgpu_rollout_group_dev(c.handle, batches, nb, 1000, 0))
        for c, dev, batches, (b, d, p, r) in runs:
            w = c.queue_counters()                  # synchronises the context's stream
            assert w[63] == 0 and w[40] == w[41] and w[40] > 0, (int(w[63]), int(w[40]), int(w[41]))
            ob, od, op = b.copy(), d.copy(), p.copy()
            oout, osteps = O.rollout_batch(ob, od, r, op, max_steps=1000, threads=16)
            assert (dev["ro"].host() == oout).all() and (dev["st"].host() == osteps).all()
            assert (dev["bo"].host() == ob).all() and (dev["do"].host() == od).all() and (dev["p"].host() == op).all()
    finally:
        for c, dev, _, _ in runs:
            try:
                c.synchronize()
            except Exception:
                pass
            for x in dev.values():
                x.free()
        other.close()


@pytest.mark.gpu
def test_carry_off_against_always_on_a_larger_launch(ctx):
    """20,000 playouts, threshold 0 against 64 (and the default), byte for byte; no oracle run."""
    n = 20000
    dev = _device_batch(ctx, n, 0x16CD00000000)
    try:
        ctx.set_move_carry(0)
        ref = _run_device_batch(ctx, dev, n)
        assert ref["st"].sum() > 50 * n
        for below in sorted({64, DEFAULT} - {0}):
            ctx.set_move_carry(below)
            got = _run_device_batch(ctx, dev, n)
            for key in ref:
                assert np.array_equal(got[key], ref[key]), (below, key)
        assert ctx.queue_counters()[63] == 0
    finally:
        for x in dev.values():
            x.free()


@pytest.mark.gpu
def test_the_setter_checks_its_range(ctx):
    lib = ctx.lib
    for below in (-1, 65, 1 << 20, -(1 << 31)):
        assert lib.oakgpu_set_move_carry(ctx.handle, below) != 0, below
        assert b"oakgpu_set_move_carry" in lib.oakgpu_last_error()
    for below in (0, 1, 64, DEFAULT):
        assert lib.oakgpu_set_move_carry(ctx.handle, below) == 0, below
