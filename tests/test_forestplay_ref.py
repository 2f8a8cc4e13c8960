"""CPU: the pick rule of a self-play turn (oak_amd/csrc/selfplay_pick.hpp, compiled for the host as oakgpu_selfplay_pick_host) against the
float64 restatement in tests/forestplay_ref.py, bit for bit; every refusal of oakgpu_forest_selfplay_check by its message; a record the
restatement assembles through oakgpu_frames_read.  No GPU involved."""
import struct

import numpy as np
import pytest

import forestplay_ref as R
from oak_amd._lib import OakGpuError
from oak_amd.frames import forest_selfplay_check, read_frames, selfplay_pick_host

MODES = ("e", "n", "x", "p", "e0.9-x0.1", "e0.5-n0.5")


def _strategy(rng, k):
    """A strategy over k entries: random, or a pure one (entries exactly 0 and 1: compress_prob's clamps)."""
    p = np.zeros(9)
    if rng.randint(4) == 0:
        p[rng.randint(k)] = 1.0
    else:
        x = rng.rand(k) * (rng.rand(k) < 0.7)
        if x.sum() == 0:
            x[0] = 1.0
        p[:k] = x / x.sum()
    return p


def _root_output(rng, case):
    """One random root output: (m, n, visits, values, iterations)."""
    shape = case % 8
    m, n = ((1, 1 + rng.randint(9)), (1 + rng.randint(9), 1), (9, 9), (1, 1))[shape] if shape < 4 else (1 + rng.randint(9), 1 + rng.randint(9))
    visits = np.zeros((9, 9), np.uint64)
    values = np.zeros((9, 9))
    kind = (case // 8) % 4
    if kind == 0:      # a budget spread thinly: most cells never visited
        iterations = 1 + rng.randint(12)
        for _ in range(iterations):
            visits[rng.randint(m), rng.randint(n)] += 1
    elif kind == 1:    # equal rows and columns: ties for 'x'
        per = 1 + rng.randint(5)
        visits[:m, :n] = per
        iterations = per * m * n
    else:
        visits[:m, :n] = rng.randint(0, 40, size=(m, n)) * (rng.rand(m, n) < 0.8)
        if visits.sum() == 0:
            visits[0, 0] = 1
        iterations = int(visits.sum())
    frac = rng.rand(9, 9)
    edge = (case // 32) % 3
    if edge == 1:
        frac[:] = 1.0      # every playout won: empirical value exactly 1
    elif edge == 2:
        frac[:] = 0.0      # every playout lost: exactly 0
    values[:m, :n] = (visits[:m, :n].astype(np.float64) * frac[:m, :n]).astype(np.float32)   # (sums of float leaf values)
    return m, n, visits, values, iterations


def _cases(count, seed):
    rng = np.random.RandomState(seed)
    for case in range(count):
        m, n, visits, values, iterations = _root_output(rng, case)
        yield {"m": m, "n": n, "visits": visits, "values": values, "iterations": iterations, "p1_nash": _strategy(rng, m), "p2_nash": _strategy(rng, n),
               "nash_value": (0.0, 1.0, float(rng.rand()))[case % 3], "p1_prior": _strategy(rng, m), "p2_prior": _strategy(rng, n),
               "c1": rng.randint(1, 255, 9).astype(np.uint8), "c2": rng.randint(1, 255, 9).astype(np.uint8), "rng": int(rng.randint(0, 1 << 62)) * 4 + case}


def _both(case, mode, minp):
    kw = dict(p1_nash=case["p1_nash"], p2_nash=case["p2_nash"], nash_value=case["nash_value"], p1_prior=case["p1_prior"], p2_prior=case["p2_prior"],
              p1_choices=case["c1"], p2_choices=case["c2"])
    want = R.pick(case["m"], case["n"], case["visits"], case["values"], case["iterations"], case["rng"], mode=mode, temp=1.0, minp=minp, **kw)
    try:
        got = selfplay_pick_host(case["m"], case["n"], case["visits"], case["values"], case["iterations"], case["rng"], policy_mode=mode, policy_temp=1.0,
                                 policy_min=minp, **kw)
    except OakGpuError as e:
        assert "zero policy" in str(e)
        got = None
    return want, got


def test_pick_rule_equals_the_restatement_bit_for_bit():
    seen = {"zeroed": 0, "cut": 0, "ties": 0, "m1": 0, "n1": 0, "full": 0, "zero_cells": 0, "clamp0": 0, "clamp1": 0, "total": 0}
    for k, case in enumerate(_cases(3072, 20260)):
        mode = MODES[k % len(MODES)]
        minp = (0.0, 0.0, 0.12, 0.3, 0.6)[(k // len(MODES)) % 5]
        want, got = _both(case, mode, minp)
        seen["total"] += 1
        if want is None:
            assert got is None, (k, mode, minp)
            seen["zeroed"] += 1
            continue
        assert got is not None, (k, mode, minp)
        assert struct.pack("<d", want["empirical_value"]) == struct.pack("<d", got["empirical_value"]), k
        for name in ("p1_empirical", "p2_empirical", "p1_policy", "p2_policy"):
            assert np.array(want[name]).tobytes() == got[name].tobytes(), (k, mode, minp, name)
        assert (want["i"], want["j"], want["rng"]) == (got["i"], got["j"], got["rng"]), (k, mode, minp)
        assert want["update"] == got["update"], (k, mode, minp)
        m, n = case["m"], case["n"]
        seen["m1"] += m == 1
        seen["n1"] += n == 1
        seen["full"] += m == 9 and n == 9
        seen["zero_cells"] += bool((case["visits"][:m, :n] == 0).any())
        seen["cut"] += minp > 0 and any(p == 0 for p in want["p1_policy"][:m])
        e1 = want["p1_empirical"][:m]
        seen["ties"] += "x" in mode and m > 1 and sorted(e1)[-1] == sorted(e1)[-2]
        d = R.decode_update(want["update"])
        seen["clamp0"] += d["empirical_value"] == 0
        seen["clamp1"] += d["empirical_value"] == 65535
    print(seen)
    assert all(v > 0 for v in seen.values()), seen   # every kind of case the rule distinguishes was drawn


def test_a_flat_policy_under_a_high_cut_is_a_zero_policy_on_both_sides():
    visits = np.zeros((9, 9), np.uint64)
    visits[:4, :4] = 2
    values = visits.astype(np.float64) * 0.5
    assert R.pick(4, 4, visits, values, 32, 7, mode="e", minp=0.3) is None
    with pytest.raises(OakGpuError, match="zero policy"):
        selfplay_pick_host(4, 4, visits, values, 32, 7, policy_mode="e", policy_min=0.3)
    # with the cut just below 1 / 4 the same policy survives whole
    got = selfplay_pick_host(4, 4, visits, values, 32, 7, policy_mode="e", policy_min=0.25)
    assert got["p1_policy"][:4].tolist() == [0.25] * 4 and got["rng"] == R.pick(4, 4, visits, values, 32, 7, minp=0.25)["rng"]


def test_pick_host_refuses_a_mode_it_cannot_parse():
    visits = np.ones((9, 9), np.uint64)
    for mode in ("b", "q", "e-b0.5", "e-e-e-e-e-e-e-e-e"):
        with pytest.raises(OakGpuError, match="policy mode"):
            selfplay_pick_host(2, 2, visits, visits.astype(np.float64), 4, 1, policy_mode=mode)


def test_the_seed_chain_is_the_host_loops():
    """rng = seed ^ 0x9FB21C651E98DF25; per turn the search seed is one splitmix64 draw, then one draw per side's sample -- the restatement's
    stream after a pick is pick_host's, and the draw in front of it is plain splitmix64 (known answer: seed 0's first output)."""
    assert R.splitmix64(0)[1] == 0xE220A8397B1DCDAF
    state = R.game_stream(12345)
    assert state == 12345 ^ 0x9FB21C651E98DF25
    visits = np.zeros((9, 9), np.uint64)
    visits[:3, :2] = [[3, 1], [0, 2], [5, 5]]
    values = visits * 0.25
    for _ in range(5):
        state, seed = R.splitmix64(state)
        want = R.pick(3, 2, visits, values, 16, state)
        got = selfplay_pick_host(3, 2, visits, values, 16, state)
        assert got["rng"] == want["rng"] and (got["i"], got["j"]) == (want["i"], want["j"])
        state = want["rng"]


def test_every_refusal_of_the_check_by_its_message():
    ok = dict(max_trees=64, max_iterations=64, contextual=False, iterations=16, n=4)
    forest_selfplay_check(**ok)
    forest_selfplay_check(**dict(ok, policy_mode="e0.9-x0.1"))
    forest_selfplay_check(**dict(ok, policy_mode="p", bandit="pucb", evaluator="net", has_net=True, contextual=True))
    forest_selfplay_check(**dict(ok, policy_mode="e", solve_nash=False))
    refusals = [
        (dict(keep_node=True), "keep_node is not supported"),
        (dict(policy_mode="b"), "policy mode 'b'"),
        (dict(policy_mode="e0.5-q0.5"), "unknown policy mode letter 'q'"),
        (dict(policy_min=1.5), "zero policy \\(policy_min above 1"),
        (dict(policy_mode="e0.5-n0.5", solve_nash=False), "word 'n' needs solve_nash"),
        (dict(bandit="exp3"), "forest search refuses: the Exp3 bandit is not supported"),
        (dict(bandit="ucb1"), "forest search refuses: the UCB1 bandit is not supported"),
        (dict(duration_us=1000), "forest search refuses: time budgets are not supported"),
        (dict(matrix_ucb=1), "forest search refuses: matrix_ucb is not supported"),
        (dict(iterations=65), "forest search refuses: iterations exceed the forest's max_iterations"),
        (dict(iterations=0), "forest search refuses: give an iteration budget"),
        (dict(n=65), "forest search refuses: n exceeds the forest's max_trees"),
        (dict(bandit="pucb", evaluator="net", has_net=True), "forest search refuses: PUCB needs a forest created contextual"),
        (dict(evaluator="net", has_net=False), "forest search refuses: network evaluation / PUCB priors need a network"),
        (dict(root_rolls=4), "forest search refuses: rolls must be"),
    ]
    for change, message in refusals:
        with pytest.raises(OakGpuError, match="oakgpu_forest_selfplay: .*" + message):
            forest_selfplay_check(**dict(ok, **change))


def test_the_endless_battle_check_names_the_lowest_game():
    from test_oracle_goldens import benchmark_teams
    good = np.array(benchmark_teams(), dtype=np.uint8).reshape(60)
    ghosts = np.tile(np.array([94, 95, 95, 95, 95], np.uint8), 12)   # Gengar with Hypnosis four times over, on both sides: nothing can hit a Ghost
    teams = np.stack([good, good, ghosts, good, ghosts])
    with pytest.raises(OakGpuError, match="oakgpu_forest_selfplay: game 2: EBC check failed"):
        forest_selfplay_check(64, 64, False, 16, n=5, teams=teams)
    forest_selfplay_check(64, 64, False, 16, n=2, teams=teams[:2])


def test_a_record_assembled_by_the_restatement_reads_back():
    rng = np.random.RandomState(5)
    battle = rng.randint(0, 256, 384).astype(np.uint8)
    state = R.game_stream(99)
    updates, picks = [], []
    for case in _cases(24, 77):
        state, _ = R.splitmix64(state)
        p = R.pick(case["m"], case["n"], case["visits"], case["values"], case["iterations"], state, p1_nash=case["p1_nash"], p2_nash=case["p2_nash"],
                   nash_value=case["nash_value"], p1_choices=case["c1"], p2_choices=case["c2"], mode="e0.5-n0.5")
        state = p["rng"]
        updates.append(p["update"])
        picks.append((case, p))
    record = R.assemble_record(battle, 2, updates)
    assert R.split_updates(record) == updates
    (game,) = read_frames(record + record)[:1]
    assert len(read_frames(record + record)) == 2
    assert (game["battle"] == battle).all() and game["result"] == 2 and len(game["updates"]) == len(updates)
    for u, (case, p) in zip(game["updates"], picks):
        assert (u["m"], u["n"], u["iterations"]) == (case["m"], case["n"], case["iterations"])
        assert (u["c1"], u["c2"]) == (case["c1"][p["i"]], case["c2"][p["j"]])
        assert u["empirical_value"] == R.compress_prob(p["empirical_value"]) / 65535.0
        assert u["nash_value"] == R.compress_prob(case["nash_value"]) / 65535.0
        assert [round(x * 65535) for x in u["p1_empirical"]] == [R.compress_prob(x) for x in p["p1_empirical"][:case["m"]]]
        assert [round(x * 65535) for x in u["p2_nash"]] == [R.compress_prob(x) for x in case["p2_nash"][:case["n"]]]
