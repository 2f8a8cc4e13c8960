"""No GPU: the fast-search turn rule and the refusals around it.
  1. selfplay_pick.hpp's turn prelude (through oakgpu_selfplay_prelude_host) equals the Python restatement on 1,000 streams at
     probabilities 0, 0.25 and 1; at 0 no draw is made: the stream is the one of a game without fast searches;
  2. every refusal of oakgpu_forest_selfplay_check for the fast fields, by its text;
  3. the budgets refusals (oakgpu_forest_budgets_check), naming the lowest offending tree;
  4. the seeds of tests/test_gpu_forest_fast_selfplay.py mix fast and full turns."""
import ctypes as C

import numpy as np
import pytest

import fast_search_ref as F
import forestplay_ref as R
from oak_amd import _lib
from oak_amd.frames import forest_selfplay_check, selfplay_prelude_host
from oak_amd.search import forest_budgets_check


@pytest.mark.parametrize("prob", [0.0, 0.25, 1.0])
def test_the_turn_prelude_is_the_restatements(prob):
    rng = np.random.default_rng(2024)
    fast_count = 0
    for k in range(1000):
        state = int(rng.integers(0, 1 << 63)) * 2 + (k & 1) if k else 0
        want_state, want_fast, want_seed = F.turn_prelude(state, prob)
        fast, seed, after = selfplay_prelude_host(state, prob)
        assert (fast, seed, after) == (want_fast, want_seed, want_state), (k, state)
        fast_count += fast
        if prob == 0.0:   # no draw: the seed is the stream's next output, as in a game without the fields
            assert (after, seed) == R.splitmix64(state) and not fast
    if prob == 0.25:
        assert 180 <= fast_count <= 320, fast_count      # 250 +- 5 sigma
    if prob == 1.0:
        assert fast_count == 1000                        # (uniform01 is below 1)


def test_a_negative_or_nan_probability_draws_nothing():
    for prob in (-0.5, float("nan")):
        fast, seed, after = selfplay_prelude_host(77, prob)
        assert (after, seed) == R.splitmix64(77) and not fast


def test_the_params_struct_mirrors_the_header():
    p = _lib.SelfplayParams
    assert p.fast_budget.offset == p.nodes_kept.offset + 4 and p.fast_search_prob.offset == (p.fast_budget.offset + 4 + 7) // 8 * 8
    assert p.fast_search_prob.offset % 8 == 0 and p.fast_policy_mode.offset == p.fast_search_prob.offset + 8 and p.fast_policy_mode.size == 16
    assert C.sizeof(p) == p.fast_policy_mode.offset + 16


@pytest.mark.parametrize("kw, text", [
    (dict(fast_search_prob=1.5), r"fast_search_prob must be in \[0, 1\]"),
    (dict(fast_search_prob=-0.1), r"fast_search_prob must be in \[0, 1\]"),
    (dict(fast_search_prob=float("nan")), r"fast_search_prob must be in \[0, 1\]"),
    (dict(fast_search_prob=0.5, fast_budget=65), "fast_budget exceeds the forest's max_iterations"),
    (dict(fast_search_prob=0.5, fast_policy_mode="b"), "fast_policy_mode: policy mode 'b'"),
    (dict(fast_search_prob=0.5, fast_policy_mode="e0.5-q"), "fast_policy_mode: unknown policy mode letter 'q'"),
    (dict(fast_search_prob=0.0, fast_policy_mode="b0.5"), "fast_policy_mode: policy mode 'b'"),      # (refused with fast searches off too)
    (dict(fast_search_prob=0.5, fast_policy_mode="e0.5-n0.5", solve_nash=False), "fast_policy_mode: policy mode word 'n' needs solve_nash"),
])
def test_the_check_refuses_by_name(kw, text):
    with pytest.raises(_lib.OakGpuError, match=text):
        forest_selfplay_check(8, 64, False, 16, n=4, evaluator="poke-engine", **kw)


def test_the_check_passes_what_it_should():
    forest_selfplay_check(8, 64, False, 16, n=4, evaluator="poke-engine")
    forest_selfplay_check(8, 64, False, 16, n=4, evaluator="poke-engine", fast_budget=64, fast_search_prob=1.0, fast_policy_mode="x")
    forest_selfplay_check(8, 64, False, 16, n=4, evaluator="poke-engine", fast_budget=4, fast_search_prob=0.0, fast_policy_mode="e0.5-n0.5", solve_nash=True)


def test_budgets_are_refused_by_name():
    forest_budgets_check([1, 24, 7], 24)
    forest_budgets_check([], 24)
    with pytest.raises(_lib.OakGpuError, match="the budget of tree 2 is 0"):
        forest_budgets_check([3, 1, 0, 0, 99], 24)
    with pytest.raises(_lib.OakGpuError, match=r"the budget of tree 1 \(25\) exceeds params->iterations \(24\)"):
        forest_budgets_check([24, 25, 0], 24)


def test_the_gpu_tests_seeds_mix_fast_and_full_turns():
    from test_gpu_forest_fast_selfplay import CASES, games
    for evaluator, n, iterations, fast_budget, prob in CASES:
        by_turn, by_game = F.mixing(games(n)[2], prob, 6)
        assert by_turn and by_game, evaluator
