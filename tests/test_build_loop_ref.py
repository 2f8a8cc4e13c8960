"""CPU: the host-only rules of the build network's side of self-play (include/oakgpu.h).
  1. oakgpu_selfplay_skip_host, the skip rule of the forest loop (selfplay_pick.hpp's game_is_skipped): its ends, its share at 0.5, and
     that the flag is a function of (seed, prob, built != 0) alone -- restated here on tests/forestplay_ref.py's stream;
  2. the refusals for battle_skip_prob and t1_budget (oakgpu_forest_selfplay_skip_check, which frames.forest_selfplay_check runs as the
     _build calls do), by their text;
  3. _lib.SelfplaySkip mirrors oakgpu_selfplay_skip, and oakgpu_selfplay_params keeps its size;
  4. oakgpu_build_game_targets_host on every status, result and seat; 5. the build window's refusals that need no device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import forestplay_ref as R
from oak_amd import _lib
from oak_amd.frames import forest_selfplay_check, selfplay_skip_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP_STREAM_XOR = 0x5B1D7C83A46E20F9
SEEDS = [(g * 0x9E3779B97F4A7C15 + 11) & 0xFFFFFFFFFFFFFFFF for g in range(4096)]


def restated(seed, prob, built):
    if not built or not prob > 0:
        return False
    return R.uniform01(seed ^ SKIP_STREAM_XOR)[1] < prob


# ---- 1. the skip rule --------------------------------------------------------------------------------------------------------------------
def test_probability_zero_or_no_built_seat_never_skips():
    for seed in SEEDS[:512]:
        assert not any(selfplay_skip_host(seed, 0.0, b) for b in (0, 1, 2, 3))
        assert not any(selfplay_skip_host(seed, p, 0) for p in (0.5, 1.0, math.nan, -1.0))
        assert not selfplay_skip_host(seed, math.nan, 3) and not selfplay_skip_host(seed, -0.5, 3)


def test_probability_one_with_a_built_seat_always_skips():
    assert all(selfplay_skip_host(seed, 1.0, b) for seed in SEEDS[:512] for b in (1, 2, 3))


def test_the_share_at_one_half_is_a_fair_coins():
    share = sum(selfplay_skip_host(seed, 0.5, 1) for seed in SEEDS) / len(SEEDS)
    print("skipped share at 0.5 over %d seeds: %.4f" % (len(SEEDS), share))
    assert abs(share - 0.5) <= 0.04      # 5 sigma of a fair coin at n = 4,096 (sigma = 0.0078): the margin guards the rule, not the generator


def test_the_flag_is_a_function_of_seed_probability_and_builtness_alone():
    for seed in SEEDS[:1024]:
        for prob in (0.1, 0.5, 0.9):
            want = restated(seed, prob, 1)
            assert [selfplay_skip_host(seed, prob, b) for b in (1, 2, 3, 255)] == [want] * 4, (seed, prob)
            assert selfplay_skip_host(seed, prob, 1) == want                     # and again: no state is kept between calls
    assert SKIP_STREAM_XOR != R.GAME_STREAM_XOR
    a = [selfplay_skip_host(seed, 0.25, 1) for seed in SEEDS[:1024]]
    b = [selfplay_skip_host(seed, 0.75, 1) for seed in SEEDS[:1024]]
    assert all(y for x, y in zip(a, b) if x) and sum(a) < sum(b)                  # one draw per seed: a larger probability skips a superset


def test_the_skip_draw_is_not_the_games_stream():
    """the first uniform of the game's own stream would give another set"""
    own = [R.uniform01(R.game_stream(seed))[1] < 0.5 for seed in SEEDS[:1024]]
    got = [selfplay_skip_host(seed, 0.5, 1) for seed in SEEDS[:1024]]
    assert own != got


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, text", [
    (dict(battle_skip_prob=-0.1), r"battle_skip_prob must be in \[0, 1\]"),
    (dict(battle_skip_prob=1.5), r"battle_skip_prob must be in \[0, 1\]"),
    (dict(battle_skip_prob=math.nan), r"battle_skip_prob must be in \[0, 1\]"),
    (dict(battle_skip_prob=0.5, t1_budget=65), "t1_budget exceeds the forest's max_iterations"),
    (dict(t1_budget=65), "t1_budget exceeds the forest's max_iterations"),
])
def test_the_check_refuses_the_skip_fields_by_name(kw, text):
    with pytest.raises(_lib.OakGpuError, match=text):
        forest_selfplay_check(8, 64, False, 16, n=4, evaluator="poke-engine", **kw)


def test_the_check_lets_the_skip_fields_pass():
    forest_selfplay_check(8, 64, False, 16, n=4, evaluator="poke-engine", battle_skip_prob=0.0, t1_budget=0)
    forest_selfplay_check(8, 64, False, 16, n=4, evaluator="poke-engine", battle_skip_prob=1.0, t1_budget=64)
    forest_selfplay_check(8, 64, False, 16, n=4, evaluator="poke-engine", battle_skip_prob=0.5, t1_budget=1, fast_budget=4, fast_search_prob=0.5)


# ---- 3. the struct ---------------------------------------------------------------------------------------------------------------------------
def test_the_skip_struct_mirrors_the_header_and_the_params_struct_keeps_its_size(tmp_path):
    src, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "oakgpu.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                         "sizeof(oakgpu_selfplay_skip), offsetof(oakgpu_selfplay_skip, t1_budget), offsetof(oakgpu_selfplay_skip, battle_skip_prob), "
                         "sizeof(oakgpu_selfplay_params), offsetof(oakgpu_selfplay_params, fast_policy_mode)); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S, P = _lib.SelfplaySkip, _lib.SelfplayParams
    assert got == [C.sizeof(S), S.t1_budget.offset, S.battle_skip_prob.offset, C.sizeof(P), P.fast_policy_mode.offset]
    assert C.sizeof(P) == P.fast_policy_mode.offset + 16        # the fields live beside the params struct, which ends where it did
    zero = S()
    assert zero.t1_budget == 0 and zero.battle_skip_prob == 0.0
    assert _lib.load().oakgpu_forest_selfplay_skip_check(16, None) == 0      # no struct: nothing is skipped, nothing to refuse


def test_the_library_exports_the_build_side_of_self_play():
    lib = _lib.load()
    for name in ("oakgpu_forest_selfplay_build_dev", "oakgpu_forest_selfplay_build", "oakgpu_forest_selfplay_matchup", "oakgpu_selfplay_skip_host",
                 "oakgpu_forest_selfplay_skip_check"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None, name


# ---- 4. the value / score rule of a game's build records ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seat", [0, 1])
@pytest.mark.parametrize("result, first", [(1, 1.0), (2, 0.0), (3, 0.5), (0x21, 1.0)])
@pytest.mark.parametrize("status", [0, 1, 2, 3])
def test_game_targets_on_every_status_result_and_seat(status, result, first, seat):
    from oak_amd import build
    for matchup in (0.0, 1.0, 0.3, 2.0 / 65535.0):
        got = build.game_targets(status, result, matchup, seat)
        if status in (1, 2):                                  # MAX_LENGTH, ZERO_POLICY: the reference's catch ... continue
            assert got is None
            continue
        value, score = got
        assert value == float(np.float32(matchup) if seat == 0 else np.float32(1.0 - matchup))
        if status == 3:                                       # SKIPPED: no battle, no score
            assert score is None
        else:
            assert score == (first if seat == 0 else 1.0 - first)


def test_game_targets_refuse_a_third_seat():
    from oak_amd import build
    with pytest.raises(_lib.OakGpuError, match="seat outside"):
        build.game_targets(0, 1, 0.5, 2)


# ---- 5. the build window's refusals that need no device ------------------------------------------------------------------------------------
def test_build_window_refusals_without_a_device():
    lib = _lib.load()
    h, size, st = C.c_void_p(), C.c_size_t(0), (C.c_uint64 * 4)()
    for call, text in [(lambda: lib.oakgpu_build_window_create(None, 0, C.byref(h)), "oakgpu_build_window_create: max_records == 0"),
                       (lambda: lib.oakgpu_build_window_create(None, 1 << 31, C.byref(h)), "max_records above"),
                       (lambda: lib.oakgpu_build_window_create(None, 64, C.byref(h)), "oakgpu_build_window_create: null argument"),
                       (lambda: lib.oakgpu_build_window_append_dev(None, None, None, None, 4), "oakgpu_build_window_append_dev: null argument"),
                       (lambda: lib.oakgpu_build_window_append(None, None, None, 128), "oakgpu_build_window_append: null argument"),
                       (lambda: lib.oakgpu_build_window_records(None, None, 0, C.byref(size)), "oakgpu_build_window_records: null argument"),
                       (lambda: lib.oakgpu_build_window_stats(None, C.byref(st)), "oakgpu_build_window_stats: null argument"),
                       (lambda: lib.oakgpu_build_game_records_dev(None, None, None, None, None, None, 1, None, None), "oakgpu_build_game_records_dev: null argument")]:
        with pytest.raises(_lib.OakGpuError, match=text):
            _lib.check(call())
    assert not h and lib.oakgpu_build_window_corpus(None) is None
    lib.oakgpu_build_window_destroy(None)
