"""CPU: one seat's pick and early-stop sign of a match between two search agents (oakgpu_match_pick_host: forestmatch.hip's rule compiled for
the host) against the float64 referee in tests/forest_match_ref.py, bit for bit; every refusal of oakgpu_forest_match_check by its message;
the struct sizes and offsets the ctypes face assumes.  No GPU involved."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import forest_match_ref as M
from oak_amd import _lib
from oak_amd._lib import OakGpuError
from oak_amd.arena import TURN_DTYPE, forest_match_check, match_pick_host
from test_forestplay_ref import _cases

MODES = ("e", "n", "x", "p", "e0.9-x0.1", "e0.5-n0.5", "p0.5-n0.5")


def _one(case, side, mode, temp, minp, early_stop):
    k = case["n"] if side else case["m"]
    nash, prior = (case["p2_nash"], case["p2_prior"]) if side else (case["p1_nash"], case["p1_prior"])
    want = M.seat_pick(side, case["m"], case["n"], case["visits"], case["values"], case["iterations"], case["rng"], nash=nash, prior=prior, mode=mode,
                       temp=temp, minp=minp, early_stop=early_stop)
    try:
        got = match_pick_host(side, case["m"], case["n"], case["visits"], case["values"], case["iterations"], case["rng"], nash=nash, prior=prior,
                              policy_mode=mode, policy_temp=temp, policy_min=minp, early_stop=early_stop)
    except OakGpuError as e:
        assert "zero policy" in str(e)
        got = None
    return k, want, got


def test_a_seats_pick_equals_the_referee_bit_for_bit():
    seen = {"zeroed": 0, "cut": 0, "temp": 0, "ev0": 0, "ev1": 0, "plus": 0, "minus": 0, "none": 0, "total": 0}
    seen.update({"k%d" % k: 0 for k in range(1, 10)})
    seen.update({"side%d" % s: 0 for s in (0, 1)})
    seen.update({"mode_" + w: 0 for w in MODES})
    for q, case in enumerate(_cases(4096, 20261)):
        side = q & 1
        mode = MODES[(q // 2) % len(MODES)]
        temp = (1.0, 1.0, 0.5, 2.0)[(q // 14) % 4]
        minp = (0.0, 0.0, 0.12, 0.3, 0.6)[(q // 56) % 5]
        early_stop = (0.0, 0.5, 10.0, 2.0)[(q // 3) % 4]
        k, want, got = _one(case, side, mode, temp, minp, early_stop)
        seen["total"] += 1
        if want is None:
            assert got is None, (q, mode, minp)
            seen["zeroed"] += 1
            continue
        assert got is not None, (q, mode, minp)
        assert struct.pack("<d", want["empirical_value"]) == struct.pack("<d", got["empirical_value"]), q
        assert np.array(want["policy"]).tobytes() == got["policy"].tobytes(), (q, mode, temp, minp)
        assert (want["index"], want["rng"], want["sign"]) == (got["index"], got["rng"], got["sign"]), (q, mode, temp, minp, early_stop)
        seen["k%d" % k] += 1
        seen["side%d" % side] += 1
        seen["mode_" + mode] += 1
        seen["temp"] += temp != 1.0
        seen["cut"] += minp > 0 and any(p == 0 for p in want["policy"][:k])
        seen["ev0"] += want["empirical_value"] == 0.0 and early_stop > 0
        seen["ev1"] += want["empirical_value"] == 1.0 and early_stop > 0
        seen["plus"] += want["sign"] > 0
        seen["minus"] += want["sign"] < 0
        seen["none"] += want["sign"] == 0 and early_stop > 0
    print(seen)
    assert all(v > 0 for v in seen.values()), seen   # every kind of case the rule distinguishes was drawn


def _root(ev_num, iterations):
    """A 2 x 2 root whose empirical value is exactly ev_num / iterations."""
    visits = np.zeros((9, 9), np.uint64)
    values = np.zeros((9, 9))
    visits[0, 0], visits[1, 1] = iterations // 2, iterations - iterations // 2
    values[0, 0] = float(ev_num)
    return visits, values


def test_the_early_stop_sign_at_its_edges():
    # ev exactly 1 and 0: t = +-inf, whatever the divisor
    for ev_num, sign in ((64, 1), (0, -1)):
        visits, values = _root(ev_num, 64)
        for early_stop in (0.5, 10.0, 1e300):
            for side in (0, 1):
                got = match_pick_host(side, 2, 2, visits, values, 64, 5, early_stop=early_stop)
                assert got["empirical_value"] == ev_num / 64 and got["sign"] == sign == M.early_stop_sign(ev_num / 64, early_stop)
        assert match_pick_host(0, 2, 2, visits, values, 64, 5, early_stop=0.0)["sign"] == 0       # off
    # just inside and just outside the threshold: logit(ev) against early_stop = logit(48 / 64) = log 3, one ulp either way
    visits, values = _root(48, 64)
    t = math.log(0.75) - math.log(0.25)
    inside, outside = np.nextafter(t, 0.0), np.nextafter(t, 2.0)
    assert match_pick_host(0, 2, 2, visits, values, 64, 5, early_stop=t)["sign"] == 1 == M.early_stop_sign(0.75, t)
    assert match_pick_host(0, 2, 2, visits, values, 64, 5, early_stop=float(inside))["sign"] == 1 == M.early_stop_sign(0.75, float(inside))
    assert match_pick_host(0, 2, 2, visits, values, 64, 5, early_stop=float(outside))["sign"] == 0 == M.early_stop_sign(0.75, float(outside))
    visits, values = _root(16, 64)
    assert match_pick_host(1, 2, 2, visits, values, 64, 5, early_stop=t)["sign"] == -1 == M.early_stop_sign(0.25, t)
    assert match_pick_host(1, 2, 2, visits, values, 64, 5, early_stop=float(outside))["sign"] == 0 == M.early_stop_sign(0.25, float(outside))
    # ev in a sweep across both thresholds of early_stop = 0.5
    for num in range(0, 65):
        visits, values = _root(num, 64)
        assert match_pick_host(0, 2, 2, visits, values, 64, 9, early_stop=0.5)["sign"] == M.early_stop_sign(num / 64, 0.5), num


def test_a_seat_draws_once_and_only_for_its_own_side():
    visits = np.zeros((9, 9), np.uint64)
    visits[:3, :2] = [[3, 1], [0, 2], [5, 5]]
    values = visits * 0.25
    state = M.R.game_stream(777)
    for side in (0, 1, 0, 1):
        want = M.seat_pick(side, 3, 2, visits, values, 16, state)
        got = match_pick_host(side, 3, 2, visits, values, 16, state)
        assert want["rng"] == got["rng"] == M.R.splitmix64(state)[0] and want["index"] == got["index"] < (2 if side else 3)
        assert got["policy"][2 if side else 3:].tolist() == [0.0] * (7 if side else 6)
        state = want["rng"]


def test_pick_host_refuses_what_it_cannot_state():
    visits = np.ones((9, 9), np.uint64)
    values = visits.astype(np.float64)
    for mode in ("b", "q", "e-b0.5", "e-e-e-e-e-e-e-e-e"):
        with pytest.raises(OakGpuError, match="policy mode"):
            match_pick_host(0, 2, 2, visits, values, 4, 1, policy_mode=mode)
    with pytest.raises(OakGpuError, match="side must be 0 or 1"):
        match_pick_host(2, 2, 2, visits, values, 4, 1)
    with pytest.raises(OakGpuError, match="early_stop must be >= 0"):
        match_pick_host(0, 2, 2, visits, values, 4, 1, early_stop=-1.0)
    flat = np.zeros((9, 9), np.uint64)
    flat[:4, :4] = 2
    with pytest.raises(OakGpuError, match="zero policy"):
        match_pick_host(0, 4, 4, flat, flat * 0.5, 32, 7, policy_min=0.3)
    assert M.seat_pick(0, 4, 4, flat, flat * 0.5, 32, 7, minp=0.3) is None


def test_every_refusal_of_the_check_by_its_message():
    good = dict(iterations=16, bandit="ucb", evaluator="poke-engine")
    ok = dict(max_trees=64, max_iterations=64, contextual=False, n=4)
    forest_match_check(seats=(good, dict(good, iterations=8, evaluator="mc", policy_mode="e0.9-x0.1")), **ok)
    forest_match_check(seats=(dict(good, bandit="pucb", evaluator="net", has_net=True, policy_mode="p0.5-n0.5"), good), **dict(ok, contextual=True))
    forest_match_check(seats=(good, good), early_stop=10.0, solve_nash=False, **ok)
    refusals = [
        (dict(policy_mode="b"), {}, "policy mode 'b'"),
        (dict(policy_mode="e0.5-q0.5"), {}, "unknown policy mode letter 'q'"),
        (dict(policy_min=1.5), {}, "zero policy \\(policy_min above 1"),
        (dict(policy_mode="e0.5-n0.5"), dict(solve_nash=False), "word 'n' needs solve_nash"),
        (dict(bandit="exp3"), {}, "the forest search refuses: the Exp3 bandit is not supported"),
        (dict(bandit="pexp3"), {}, "the forest search refuses: the PExp3 bandit is not supported"),
        (dict(bandit="ucb1"), {}, "the forest search refuses: the UCB1 bandit is not supported"),
        (dict(duration_us=1000), {}, "the forest search refuses: time budgets are not supported"),
        (dict(matrix_ucb=1), {}, "the forest search refuses: matrix_ucb is not supported"),
        (dict(iterations=65), {}, "the forest search refuses: iterations exceed the forest's max_iterations"),
        (dict(iterations=0), {}, "the forest search refuses: give an iteration budget"),
        (dict(root_rolls=4), {}, "the forest search refuses: rolls must be"),
        (dict(bandit="pucb", evaluator="net", has_net=True), {}, "the forest search refuses: PUCB needs a forest created contextual"),
        (dict(evaluator="net", has_net=False), {}, "the forest search refuses: network evaluation / PUCB priors need a network"),
    ]
    for change, call, message in refusals:
        for seat in (0, 1):                      # either seat is refused, by its name
            seats = [good, good]
            seats[seat] = dict(good, **change)
            with pytest.raises(OakGpuError, match="oakgpu_forest_match: seat p%d: .*%s" % (seat + 1, message)):
                forest_match_check(seats=tuple(seats), **dict(ok, **call))
    with pytest.raises(OakGpuError, match="oakgpu_forest_match: n exceeds the forest's max_trees"):
        forest_match_check(seats=(good, good), **dict(ok, n=65))
    for bad in (-1.0, float("nan")):
        with pytest.raises(OakGpuError, match="oakgpu_forest_match: early_stop must be >= 0"):
            forest_match_check(seats=(good, good), early_stop=bad, **ok)


def test_eight_words_pass_and_a_ninth_is_refused():
    """Eight words fill a seat's 16-byte mode field (it may lack its terminator) and pass the check; nine one-letter words need 17
    characters, so the field cannot hold them and the word limit is met through pick_host's free-length string."""
    from oak_amd.arena import _match_seat
    good = dict(iterations=16, bandit="ucb", evaluator="poke-engine")
    p = _lib.ForestMatchParams(_match_seat(good), _match_seat(good), 0, 0.0, 0, 1)
    C.memmove(C.addressof(p) + _lib.ForestMatchParams.p2.offset + _lib.MatchSeat.policy_mode.offset, b"e-x-e-x-e-x-e-x9", 16)
    assert _lib.load().oakgpu_forest_match_check(64, 64, 0, C.byref(p), 4) == 0
    visits = np.ones((9, 9), np.uint64)
    with pytest.raises(OakGpuError, match="8 at the most"):
        match_pick_host(0, 2, 2, visits, visits.astype(np.float64), 4, 1, policy_mode="e-e-e-e-e-e-e-e-e")


def test_the_struct_layouts_the_ctypes_face_assumes():
    S, P, T = _lib.MatchSeat, _lib.ForestMatchParams, _lib.MatchTurn
    assert C.sizeof(_lib.SearchParams) == 80
    assert (S.search.offset, S.net.offset, S.policy_mode.offset, S.policy_temp.offset, S.policy_min.offset, C.sizeof(S)) == (0, 80, 88, 104, 112, 120)
    assert (P.p1.offset, P.p2.offset, P.max_turns.offset, P.early_stop.offset, P.log_turns.offset, P.solve_nash.offset, C.sizeof(P)) == \
        (0, 120, 240, 248, 256, 260, 264)
    assert (T.c1.offset, T.c2.offset, T.m.offset, T.n.offset, T.zero.offset, T.ev_p1.offset, T.ev_p2.offset, C.sizeof(T)) == (0, 1, 2, 3, 4, 8, 16, 24)
    assert TURN_DTYPE.itemsize == 24 and [TURN_DTYPE.fields[k][1] for k in ("c1", "c2", "m", "n", "zero", "ev_p1", "ev_p2")] == [0, 1, 2, 3, 4, 8, 16]
    # the library reads the same layout: a params block built here passes the check, and one with p2's budget out of range names p2
    from oak_amd.arena import _match_seat
    good = dict(iterations=16, bandit="ucb", evaluator="poke-engine")
    p = P(_match_seat(good), _match_seat(dict(good, iterations=65)), 0, 0.0, 0, 1)
    assert _lib.load().oakgpu_forest_match_check(64, 64, 0, C.byref(p), 4) != 0
    assert b"seat p2" in _lib.load().oakgpu_last_error()
    p.early_stop = -2.0
    p.p2.search.iterations = 16
    assert _lib.load().oakgpu_forest_match_check(64, 64, 0, C.byref(p), 4) != 0
    assert b"early_stop" in _lib.load().oakgpu_last_error()
