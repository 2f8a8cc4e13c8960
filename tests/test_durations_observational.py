"""The chance-durations word is observational: the caller's hidden-variable resampling (prep) and the leaf network's encoder read it,
the engine's transitions never do.  That is what lets a rollout launch which hands no durations back keep none (EngineR's KEEP_DUR,
k_rollout_queue's lean instantiation).  Held here on the CPU oracle alone: 4,096 random OU playouts advanced 25 turn-steps, then
played to the end once from their real durations and once from zeroed ones."""
import numpy as np

import lean_ref as L

N, SEED0 = 4096, 0x0A4B00000000
KEYS = ("results", "steps", "battles", "prng")


def _inputs():
    b, d, p, r = L.midgame(N, SEED0)
    lanes, attacking, binding = L.census(d, r)
    print("running lanes with non-zero durations %d, sides with an attacking count %d, with a binding count %d" % (lanes, attacking, binding))
    assert lanes >= 200 and attacking >= 100 and binding >= 10, (lanes, attacking, binding)
    return b, d, p, r


def test_without_prep_nothing_but_the_durations_depends_on_the_durations():
    b, d, p, r = _inputs()
    real, zeroed = L.play(b, d, p, r), L.play(b, np.zeros_like(d), p, r)
    for key in KEYS:
        bad = real[key] != zeroed[key]
        assert not bad.any(), (key, int(bad.reshape(N, -1).any(axis=1).sum()))
    assert (real["durations"] != zeroed["durations"]).any()  # (the word itself is carried, and differs)


def test_with_prep_the_durations_are_read_once():
    b, d, p, r = _inputs()
    real, zeroed = L.play(b, d, p, r, prep=True), L.play(b, np.zeros_like(d), p, r, prep=True)
    assert any((real[key] != zeroed[key]).any() for key in KEYS)
