"""Mid-game inputs with non-zero chance durations, shared by the tests of the durations-free rollout (tests/test_durations_observational.py,
tests/test_gpu_lean_rollout.py, tests/test_gpu_lean_root_step.py).  A fresh battle's durations are all zero and cannot tell a stale
load of the word from none, so every input here is a playout the oracle has advanced a few turn-steps."""
import functools

import numpy as np

import oracle_lib as O

SLEEP_BITS, CONFUSION, DISABLE, ATTACKING, BINDING = (1 << 18) - 1, 7 << 18, 15 << 21, 7 << 25, 7 << 28


@functools.lru_cache(maxsize=None)
def midgame(n, seed0, advance=25):
    """n random OU playouts advanced `advance` turn-steps by the oracle: read-only (battles, durations, prng, results)."""
    b, d, p, r = O.make_random_ou_batch(n, seed0=seed0)
    res, _ = O.rollout_batch(b, d, r, p, max_steps=advance, threads=8)
    out = (b, d, p, res)
    for a in out:
        a.setflags(write=False)
    return out


def census(durations, results):
    """(running lanes with a non-zero durations word, sides of them with an attacking count, ... with a binding count)."""
    w = np.ascontiguousarray(durations).view(np.uint32).reshape(-1, 2)[(np.asarray(results) & 15) == 0]
    return int((w != 0).any(axis=1).sum()), int(((w & ATTACKING) != 0).sum()), int(((w & BINDING) != 0).sum())


def play(b, d, p, r, max_steps=1000, prep=False):
    """The oracle's playouts from copies of the inputs: dict of results, steps, values, battles, durations, prng."""
    ob, od, op = b.copy(), d.copy(), p.copy()
    out, steps = O.rollout_batch(ob, od, np.ascontiguousarray(r), op, max_steps=max_steps, prep=prep, threads=8)
    t = out & 15
    return dict(results=out, steps=steps, values=np.where(t == 1, 1.0, np.where(t == 2, 0.0, 0.5)).astype(np.float32), battles=ob,
                durations=od, prng=op)
