"""CPU: the helpers the whole-game tests are built on (tests/policy_games_ref.py) -- the Python fast_prng against the reference's known
answers and the oracle's streams, the policy rule's edge cases, and the share of picks a GPU test may leave out."""
import json
import os

import numpy as np

import oracle_lib as O
import policy_games_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KA = json.load(open(os.path.join(ROOT, "tests", "golden", "rng_known_answers.json")))["fast_prng"]


def test_python_stream_matches_the_reference_known_answers():
    for seed, v in KA.items():
        g = R.FastPrng(v["state"])
        assert [str(g.uniform_64()) for _ in range(len(v["uniform_64"]))] == v["uniform_64"], seed
        assert [g.next32() % 9 for _ in range(len(v["random_int_9"]))] == v["random_int_9"], seed
        if "uniform" in v:
            assert [g.uniform() for _ in range(len(v["uniform"]))] == v["uniform"], seed
        assert g.state().shape == (8,)


def test_python_stream_follows_the_oracle_rollout():
    """16 lanes: one uniform_64 per turn-step, so the oracle's final PRNG state is the Python stream advanced `steps` times."""
    b, d, p, r = O.make_random_ou_batch(16, seed0=0x9A3E5)
    start = p.copy()
    out, steps = O.rollout_batch(b, d, r, p, max_steps=1000)
    for i in range(16):
        g = R.FastPrng(start[i])
        for _ in range(int(steps[i])):
            g.uniform_64()
        assert (g.state() == p[i]).all(), i
    assert (steps > 0).all()


def test_policy_rule_edge_cases():
    F = np.float32
    # k = 1: the whole mass, whatever the logit, temp or min
    assert R.policy([F(-3.5)]).tolist() == [1.0]
    assert R.policy([F(7.0)], temp=0.5, minp=0.9).tolist() == [1.0]
    # the plain rule: expf, fp32 sum in index order, double quotient
    l = np.array([0.25, -1.0, 2.0], F)
    ex = np.exp(l)
    s = F(F(ex[0] + ex[1]) + ex[2])
    assert (R.policy(l) * np.float64(s) / ex.astype(np.float64) - 1.0).max() < 1e-15
    # min zeroes all but one: that one gets everything
    p = R.policy(np.array([0.0, 3.0, 0.1], F), minp=0.5)
    assert p.tolist() == [0.0, 1.0, 0.0]
    # min above every entry: a zero policy
    assert R.policy(np.array([0.0, 0.0], F), minp=0.6) is None
    # temp with an entry that is exactly zero (expf underflows): pow(0, temp) = 0, the rest renormalised
    p = R.policy(np.array([-200.0, 0.0, 0.0], F), temp=0.5)
    assert p[0] == 0.0 and abs(p[1] - 0.5) < 1e-15 and abs(p[2] - 0.5) < 1e-15
    # temp sharpens / flattens: sqrt of (0.8, 0.2), renormalised
    base = R.policy(np.log(np.array([0.8, 0.2], F)))
    flat = R.policy(np.log(np.array([0.8, 0.2], F)), temp=0.5)
    want = np.sqrt(base) / np.sqrt(base).sum()
    assert np.abs(flat - want).max() < 1e-15
    # sample_pdf: first index whose running difference is <= 0; a draw of exactly 0 takes index 0; rounding past the end falls back to 0
    assert R.sample_pdf([0.25, 0.5, 0.25], 0.0) == 0
    assert R.sample_pdf([0.25, 0.5, 0.25], 0.25) == 0
    assert R.sample_pdf([0.25, 0.5, 0.25], 0.2500001) == 1
    assert R.sample_pdf([0.25, 0.5, 0.25], 0.99) == 2
    assert R.sample_pdf([0.25, 0.5, 0.2], 0.99) == 0
    # a POLICY seat with one choice draws nothing; a RANDOM seat beside it draws one uniform_64
    g, h = R.FastPrng(KA["0"]["state"]), R.FastPrng(KA["0"]["state"])
    (i1, p1, u1), (i2, p2, u2) = R.turn_draws(((R.POLICY, 1.0, 0.0), (R.RANDOM, 0, 0)), g, 1, 4, np.zeros(9, F), None)
    assert (i1, p1, u1) == (0, None, None) and i2 == h.uniform_64() % 4 and (g.state() == h.state()).all()


def test_exclusion_share_is_far_below_the_cap():
    """100,000 synthetic picks: with uniform draws and at most 8 interior boundaries the share within 1e-5 of one is below
    2 x 8 x 1e-5 = 1.6e-4 in expectation -- at most 16 of these picks, and 32 is four standard deviations above that; the GPU tests allow 1 %."""
    share = R.exclusion_share(100000, np.random.default_rng(5), R.FastPrng(KA["1111111"]["state"]))
    print("share of picks within %g of a boundary: %.2e" % (R.BOUNDARY_EPS, share))
    assert share <= 3.2e-4
