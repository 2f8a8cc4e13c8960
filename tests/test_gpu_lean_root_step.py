"""k_root_step's durations-free instantiation (a handle made while oakgpu_set_lean_rollout is on): the step returns per-root
aggregates only, so a fresh playout's durations serve its prep and nothing after, and a carried playout's record holds none.  The
aggregates of every step, the turn-steps every launch executes and the lane streams must equal the oracle's (O.root_steps_reference)
and be byte-identical with the setter on and off.  What can go wrong: a prep that reads no or stale durations, a carry record whose
fields land in the wrong registers when it is resumed (the two instantiations lay the sides out differently).

Smallest shape: 4 roots x 256 playouts, slices of 4 and 16 turn-steps, 6 steps -- the carried playouts cross at least two launches.
The roots are mid-game states with non-zero durations, so prep has something to read."""
import os
import re

import numpy as np
import pytest

import lean_ref as L
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAN_DEFAULT = int(re.search(r"#define\s+OAKGPU_LEAN_ROLLOUT_DEFAULT\s+(\d+)", open(os.path.join(ROOT, "include", "oakgpu.h")).read()).group(1))
ROOTS, REPS, STEPS = 4, 256, 6


def _roots():
    """Four running mid-game states: one with an attacking or binding count, the others with any non-zero durations word."""
    b, d, p, r = L.midgame(256, 0x32B00000)
    w = d.view(np.uint32).reshape(-1, 2)
    running = (r & 15) == 0
    locked = np.where(running & ((w & (L.ATTACKING | L.BINDING)) != 0).any(axis=1))[0]
    other = np.where(running & (w != 0).any(axis=1) & ((w & (L.ATTACKING | L.BINDING)) == 0).all(axis=1))[0]
    assert len(locked) >= 1 and len(other) >= ROOTS - 1
    pick = np.concatenate([locked[:1], other[:ROOTS - 1]])
    return tuple(np.ascontiguousarray(x[pick]) for x in (b, d, r))


def _run(ctx, lean, b, d, r, lane, slice_, cnt):
    from test_gpu_parity import _RootSteps
    ctx.set_lean_rollout(lean)      # (read when the handle is made)
    rs = _RootSteps(ctx, b, d, r, lane, REPS, slice_)
    recs = []
    try:
        k = 0
        while True:
            rec = rs.step(fresh=k < STEPS)
            assert rec["err"] == 0
            recs.append((rec["count"], rec["sum2"], rec["turn_steps"], rec["carried"]))
            k += 1
            if k >= STEPS and rec["carried"] == 0:
                break
            assert k < cnt.shape[0], "playouts still in flight after the longest possible life"
        return recs, rs.lane_streams()
    finally:
        rs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slice_", (4, 16))
def test_aggregates_with_and_without_durations(gpu_ctx, slice_):
    from test_gpu_parity import _seed_prng
    b, d, r = _roots()
    lane = _seed_prng(ROOTS * REPS, 0xC40000000000)
    ref_lane = lane.copy()
    cnt, s2, ex = O.root_steps_reference(b, d, r, ref_lane, REPS, STEPS, slice_, threads=8)
    # prep matters for these roots: from zeroed durations the oracle credits other aggregates
    zc, zs, _ = O.root_steps_reference(b, np.zeros_like(d), r, lane.copy(), REPS, STEPS, slice_, threads=8)
    assert (zc != cnt).any() or (zs != s2).any(), "the roots' durations do not reach the aggregates"
    try:
        runs = {lean: _run(gpu_ctx, lean, b, d, r, lane.copy(), slice_, cnt) for lean in (1, 0)}
    finally:
        gpu_ctx.set_lean_rollout(LEAN_DEFAULT)
    for lean, (recs, streams) in runs.items():
        carried_launches = sum(1 for rec in recs if rec[3] > 0)
        assert carried_launches >= 2, "no playout crossed two launches"
        for k, (count, sum2, turn_steps, _) in enumerate(recs):
            assert (count == cnt[k]).all(), (lean, k, count, cnt[k])
            assert (sum2 == s2[k]).all(), (lean, k)
            assert turn_steps == ex[k], (lean, k, turn_steps, ex[k])
        assert cnt[len(recs):].sum() == 0 and cnt[:len(recs)].sum() == ROOTS * REPS * STEPS
        assert (streams == ref_lane).all()
    (a, sa), (c, sc) = runs[1], runs[0]
    assert len(a) == len(c) and all((x[0] == y[0]).all() and (x[1] == y[1]).all() and x[2] == y[2] and x[3] == y[3] for x, y in zip(a, c))
    assert (sa == sc).all()
