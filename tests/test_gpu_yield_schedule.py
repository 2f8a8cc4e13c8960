"""The yielding schedule of group launches (oakgpu_set_yield_schedule): the launch runs R waves fewer than it would, a dry wave with
few playing lanes parks them (the regrouping rounds' bit-exact image) and leaves, and one follow-up dispatch of at most R waves
finishes the parked playouts.  Results are indexed by playout, so every output byte must equal the CPU oracle's whichever dispatch
finishes a playout.  What can go wrong: a parked playout resumed twice or never, resumed with another playout's image or durations
or with a stale choice stream, and a context that takes the schedule when it runs alone or misses it when it alternates.

Small launches: 2 x 4,096 playouts at two playouts per lane are 64 waves, 48 for the first dispatch and 16 for the follow-up in
mode 2; automatic mode reaches them with the saturation test lowered (oakgpu_set_yield_saturation).  Lane spread off."""
import functools

import numpy as np
import pytest

import lean_ref as L
import oracle_lib as O

VALUE_KEYS = ("results", "steps", "values", "prng")
STATE_KEYS = VALUE_KEYS + ("battles",)
N = 4096
BELOW = 32   # a dry wave parks fewer than 32 playing lanes


@functools.lru_cache(maxsize=None)
def _fresh():
    out = tuple(O.make_random_ou_batch(N, seed0=0x33A00000 + 7919 * k) for k in range(2))
    for batch in out:
        for a in batch:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _fresh_oracle(max_steps, prep):
    return [L.play(b, d, p, r, max_steps, prep=bool(prep)) for b, d, p, r in _fresh()]


def _midgame():
    return [L.midgame(N, 0x33A10000 + 7919 * k) for k in range(2)]


@functools.lru_cache(maxsize=None)
def _midgame_oracle(max_steps):
    return [L.play(b, d, p, r, max_steps) for b, d, p, r in _midgame()]


def _prepare(c):
    from oak_amd import _lib
    c.set_playouts_per_lane(2)
    _lib.check(c.lib.oakgpu_set_spread(c.handle, 0))
    return c


def _restore(c):
    from oak_amd import _lib
    c.set_playouts_per_lane(2)
    _lib.check(c.lib.oakgpu_set_spread(c.handle, -1))
    c.set_yield_schedule(0)
    c.set_yield_saturation(0)
    c.set_migration(1, 300, 0)
    c.set_lean_rollout(True)


@pytest.fixture
def ctx(gpu_ctx):
    try:
        yield _prepare(gpu_ctx)
    finally:
        _restore(gpu_ctx)


def _same(got, exp, keys, what):
    for k, (g, e) in enumerate(zip(got, exp)):
        for key in keys:
            bad = g[key] != e[key]
            assert not bad.any(), (what, "batch %d" % k, key, int(bad.reshape(len(bad), -1).any(axis=1).sum()))


def _launch(c, batches, max_steps=1000, prep=False, full=True):
    """One group launch: `full` takes the final battles of both batches and the durations of the first back (the kernel that keeps
    durations); otherwise values only (the lean kernels)."""
    got = c.rollout_group([(b, d, r, p) for b, d, p, r in batches], max_steps=max_steps, prep=prep, return_state=full,
                          return_durations=(True, False) if full else False)
    assert c.last_launch_lean() == (not full)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("prep", (0, 1))
@pytest.mark.parametrize("max_steps", (17, 1000))
def test_mode_2_on_one_context(ctx, max_steps, prep):
    """Every group launch yields: the full kernel and the lean ones, fresh playouts and root prep, at the smallest cap the queue kernel
    runs and at the full one.  Every playout is finished exactly once: a second finish would advance its choice stream twice."""
    ctx.set_yield_schedule(2, BELOW, 0, 8)
    exp = _fresh_oracle(max_steps, prep)
    for full in (True, False):
        got = _launch(ctx, _fresh(), max_steps, bool(prep), full)
        assert ctx.last_launch_yield()
        parked = ctx.last_launch_parked()
        print("cap %d prep %d full %d: parked %d of %d" % (max_steps, prep, full, parked, 2 * N))
        assert 0 < parked <= 2 * N, "no lane was parked: the launch proves nothing"
        _same(got, exp, STATE_KEYS if full else VALUE_KEYS, (max_steps, prep, full))
        assert all((g["steps"] > 0).all() for g in got), "a playout was never written"   # (the arrays start as zeros)
        if full:
            assert (got[0]["durations"] == exp[0]["durations"]).all()
        assert ctx.queue_counters()[63] == 0


@pytest.mark.gpu
def test_two_contexts_alternating_in_mode_1():
    """Three launches each, A B A B A B: no context yields on its first launch (nobody has launched since its previous one), every later
    launch does; the outputs are those of the same launches with the schedule off, and the oracle's."""
    from oak_amd.engine import Context
    a, b = _prepare(Context(0)), _prepare(Context(0))
    try:
        exp = _fresh_oracle(1000, 0)
        off = []
        for k in range(6):   # (schedule off and the device's own saturation test: these launches do not count as saturating ones)
            c = (a, b)[k % 2]
            c.set_yield_schedule(0)
            off.append(_launch(c, _fresh(), full=k % 3 == 0))
            assert not c.last_launch_yield() and c.last_launch_parked() == 0
        for c in (a, b):
            c.set_yield_schedule(1, BELOW, 0, 0)
            c.set_yield_saturation(32)
        for k in range(6):
            c = (a, b)[k % 2]
            got = _launch(c, _fresh(), full=k % 3 == 0)
            assert c.last_launch_yield() == (k >= 2), ("launch %d" % k, c.last_launch_yield())
            assert (c.last_launch_parked() > 0) == (k >= 2), ("launch %d" % k, c.last_launch_parked())
            keys = STATE_KEYS if k % 3 == 0 else VALUE_KEYS
            _same(got, off[k], keys, ("against the schedule off", k))
            _same(got, exp, keys, ("against the oracle", k))
            assert c.queue_counters()[63] == 0
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_midgame_inputs_with_live_durations(ctx):
    """Inputs whose durations words are live: a parked playout resumed with a stale or missing word ends with other durations (the
    kernel that keeps them) -- and the lean kernels, which park none, must not need one."""
    batches = _midgame()
    for b, d, p, r in batches:
        lanes, attacking, binding = L.census(d, r)
        assert lanes >= N // 16 and attacking >= 1, ("the inputs carry too few live durations", lanes, attacking, binding)
    exp = _midgame_oracle(1000)
    assert (exp[0]["durations"] != 0).any()
    ctx.set_yield_schedule(2, BELOW, 0, 8)
    for full in (True, False):
        got = _launch(ctx, batches, full=full)
        assert ctx.last_launch_yield() and ctx.last_launch_parked() > 0
        _same(got, exp, STATE_KEYS if full else VALUE_KEYS, ("midgame", full))
        if full:
            assert (got[0]["durations"] == exp[0]["durations"]).all()
        assert ctx.queue_counters()[63] == 0


@pytest.mark.gpu
def test_a_lone_context_in_mode_1_keeps_the_single_dispatch_with_migration():
    """Automatic mode, the saturation test lowered, nobody else launching: every launch is one dispatch, and migration (forced on for
    the small launch) donates and adopts as before."""
    from oak_amd.engine import Context
    c = _prepare(Context(0))
    try:
        c.set_yield_schedule(1, BELOW, 0, 0)
        c.set_yield_saturation(32)
        c.set_migration(2, 60, 4)
        exp = _fresh_oracle(1000, 0)
        for k in range(3):
            got = _launch(c, _fresh(), full=k == 0)
            assert not c.last_launch_yield() and c.last_launch_parked() == 0, "launch %d" % k
            w = c.queue_counters()
            assert w[63] == 0 and w[40] > 0 and w[40] == w[41], (int(w[63]), int(w[40]), int(w[41]))
            _same(got, exp, STATE_KEYS if k == 0 else VALUE_KEYS, ("lone", k))
    finally:
        c.close()


@pytest.mark.gpu
def test_the_setters_check_their_ranges(ctx):
    lib = ctx.lib
    for args in ((-1, 16, 0, 0), (3, 16, 0, 0), (1, 0, 0, 0), (1, 65, 0, 0), (1, 16, -1, 0), (1, 16, 0, 65)):
        assert lib.oakgpu_set_yield_schedule(ctx.handle, *args) != 0, args
        assert b"oakgpu_set_yield_schedule" in lib.oakgpu_last_error()
    assert lib.oakgpu_set_yield_saturation(ctx.handle, -1) != 0
    assert lib.oakgpu_set_yield_schedule(ctx.handle, 0, 16, 256, 0) == 0
