"""GPU: the exact Nash solve on the device (oak_amd/csrc/nashdev.hip; contract in include/oakgpu.h) -- bit for bit the host's.
  1. oakgpu_nash_solve_dev over the payoff kernel's row layout equals the host loops' solve per row: every shape, both widths in one launch,
     refused rows as zeros, NaN-prefilled outputs between guard bands, row counts 1, 2 and about 700;
  2. solve_matrices through ctypes, pyoak and C++ equals a loop of solve_matrix;
  3. forest_search, 4. forest_selfplay and 5. search_games with solve_nash="device" return what solve_nash=True returns;
  6. a matrix's result does not depend on its row, its neighbours or the batch size."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nash_cases as NC
from hipmem import Dev
from oak_amd import _lib
from oak_amd._lib import OakGpuError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64          # doubles on either side of the output
_CACHE = {}


def host_rows(lib, rows):
    """What the host loops' solve_rows writes for these rows: p1 [count, 9], p2 [count, 9], value / 256 [count]; zeros where the solver refuses."""
    count = len(rows)
    p1, p2, v = np.zeros((count, 9)), np.zeros((count, 9)), np.zeros(count)
    for k in range(count):
        m, n = int(rows[k, 81]) & 0xFF, (int(rows[k, 81]) >> 8) & 0xFF
        if not (1 <= m <= 9 and 1 <= n <= 9):
            continue
        M = np.ascontiguousarray(rows[k, :m * n], dtype=np.int32)
        x, y, val = np.zeros(9), np.zeros(9), np.zeros(1)
        if lib.oakgpu_solve_matrix(NC.vp(M), m, n, 256, NC.vp(x), NC.vp(y), NC.vp(val)) == 0:
            p1[k], p2[k], v[k] = x, y, val[0]
    return p1, p2, v


def device_rows(ctx, rows):
    """oakgpu_nash_solve_dev into a NaN-filled buffer with guard bands: (p1, p2, value) and the two guards' bit patterns"""
    count = len(rows)
    nan = np.full(GUARD + count * 19 + GUARD, np.nan)
    d_pay, d_out = Dev(np.ascontiguousarray(rows, dtype=np.int32)), Dev(nan)
    try:
        _lib.check(ctx.lib.oakgpu_nash_solve_dev(ctx.handle, d_pay.p, count, C.c_void_p(d_out.p.value + GUARD * 8)))
        ctx.synchronize()
        out = d_out.host()
    finally:
        d_pay.free()
        d_out.free()
    body = out[GUARD:GUARD + count * 19]
    guards = np.concatenate([out[:GUARD], out[GUARD + count * 19:]])
    assert NC.same_bits(guards, np.full(2 * GUARD, np.nan)), "a guard band was written"
    return body[:count * 9].reshape(count, 9), body[count * 9:count * 18].reshape(count, 9), body[count * 18:]


def big_batch():
    """about 700 rows: every shape with seven families (the +-2^20 ones take the wide kernel, the others the narrow one: mixed row by
    row), rock-paper-scissors, matrices at and beyond the narrow width's bound, and refused rows among them"""
    if "big" in _CACHE:
        return _CACHE["big"]
    lib = _lib.load()
    mats = NC.batch(77, {f: 1 for f in NC.FAMILIES}) + NC.batch(78, {"small": 1, "large": 1})[1:]      # 1 + 81 * 7 + 81 * 2 = 730
    bound = lib.oakgpu_nash_width4_max_entry()
    mats += [np.array([[0, bound - 1], [bound - 1, 5]]), np.array([[0, bound], [bound, 5]])]
    rows = NC.pack_rows(mats)
    refused = {}
    for at, kind in ((5, "m0"), (200, "n10"), (401, "beyond"), (650, "m0"), (0, "beyond")):
        refused[at] = kind
        if kind == "m0":
            rows[at, 81] = 0 | 3 << 8
        elif kind == "n10":
            rows[at, 81] = 2 | 10 << 8
        else:
            rows[at, 0] = (1 << 20) + 1
    _CACHE["big"] = (rows, refused, host_rows(lib, rows))
    return _CACHE["big"]


# ---- 1. the device entry point ------------------------------------------------------------------------------------------------------------------
def test_nash_solve_dev_equals_the_host_rows(gpu_ctx):
    rows, refused, (p1, p2, v) = big_batch()
    assert 650 <= len(rows) <= 760
    shapes = {(int(x) & 0xFF, (int(x) >> 8) & 0xFF) for x in rows[:, 81]}
    assert {(m, n) for m in range(1, 10) for n in range(1, 10)} <= shapes
    q1, q2, u = device_rows(gpu_ctx, rows)
    assert not np.isnan(q1).any() and not np.isnan(q2).any() and not np.isnan(u).any()       # every row is written
    assert NC.same_bits(q1, p1) and NC.same_bits(q2, p2) and NC.same_bits(u, v)
    for at in refused:
        assert not q1[at].any() and not q2[at].any() and u[at] == 0.0, (at, refused[at])
    solved = [k for k in range(len(rows)) if k not in refused]
    assert all(abs(q1[k].sum() - 1.0) < 1e-9 and abs(q2[k].sum() - 1.0) < 1e-9 for k in solved)   # the neighbours of the refused rows included
    for count in (1, 2):
        for first in (1, 6, len(rows) - 2):
            part = rows[first:first + count]
            r1, r2, r = device_rows(gpu_ctx, part)
            assert NC.same_bits(r1, p1[first:first + count]) and NC.same_bits(r2, p2[first:first + count]) and NC.same_bits(r, v[first:first + count]), (count, first)


# ---- 6. independence ------------------------------------------------------------------------------------------------------------------------------
def test_a_matrix_does_not_depend_on_its_row_or_the_batch(gpu_ctx):
    rows, refused, (p1, p2, v) = big_batch()
    rng = np.random.default_rng(3)
    pick = rng.choice([k for k in range(len(rows)) if k not in refused], 50, replace=False)
    for k in pick:
        r1, r2, r = device_rows(gpu_ctx, rows[k:k + 1])
        assert NC.same_bits(r1[0], p1[k]) and NC.same_bits(r2[0], p2[k]) and NC.same_bits(r, v[k:k + 1]), k
    for size in (7, 700):
        done = 0
        while done < 50:
            some = pick[done:done + min(size, 50)]
            where = rng.choice(size, len(some), replace=False)
            batch = rows[rng.integers(0, len(rows), size)].copy()          # other matrices all around, in another order every time
            batch[where] = rows[some]
            r1, r2, r = device_rows(gpu_ctx, batch)
            assert NC.same_bits(r1[where], p1[some]) and NC.same_bits(r2[where], p2[some]) and NC.same_bits(r[where], v[some]), (size, done)
            done += len(some)


# ---- 2. the host faces ----------------------------------------------------------------------------------------------------------------------------
def test_solve_matrices_equals_a_loop_of_solve_matrix(gpu_ctx, tmp_path):
    from oak_amd import pyoak
    from oak_amd.search import solve_matrices, solve_matrix
    mats = NC.batch(91, {"small": 1, "large": 1, "dup_row": 1})
    for factor in (256, 1):
        got = solve_matrices(gpu_ctx, mats, factor)
        assert len(got) == len(mats)
        for k, A in enumerate(mats):
            w1, w2, wv = solve_matrix(A, factor)
            assert got[k][0].shape == w1.shape and got[k][1].shape == w2.shape
            assert NC.same_bits(got[k][0], w1) and NC.same_bits(got[k][1], w2) and NC.same_bits([got[k][2]], [wv]), (k, A.shape, factor)
    assert solve_matrices(gpu_ctx, []) == []
    with pytest.raises(OakGpuError, match="matrix 1: payoffs out of range"):
        solve_matrices(gpu_ctx, [mats[0], np.array([[1 << 21]])])
    with pytest.raises(RuntimeError, match="matrix 1: payoff matrix must be between 1x1 and 9x9"):
        solve_matrices(gpu_ctx, [mats[0], np.zeros((10, 2), dtype=int)])
    floats = [A.astype(np.float32) / 256.0 for A in mats if np.abs(A).max() <= 256][:120]
    got = pyoak.solve_matrices(floats, 256)
    assert len(got) == len(floats)
    for k, F in enumerate(floats):
        w1, w2, wv = pyoak.solve_matrix(F, 256)
        assert np.asarray(got[k][0]).tobytes() == np.asarray(w1).tobytes() and np.asarray(got[k][1]).tobytes() == np.asarray(w2).tobytes(), k
        assert np.float32(got[k][2]).tobytes() == np.float32(wv).tobytes(), k
    exe = str(tmp_path / "cpp_device_nash_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_device_nash_smoke.cc"), "-L",
                           os.path.join(ROOT, "oak_amd"), "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "solve_matrices == solve_matrix" in run.stdout and run.stdout.strip().endswith("ok"), run.stdout + run.stderr


# ---- 3. the forest search -------------------------------------------------------------------------------------------------------------------------
def same_trees(got, want):
    from test_gpu_search_forest import same_output
    assert len(got) == len(want)
    for a, b in zip(got, want):
        same_output(a, b)
        assert a["stream"] == b["stream"] and a["raw"].total_depth == b["raw"].total_depth


@pytest.mark.parametrize("case", ["ucb poke-engine", "pucb tiny"])
def test_forest_search_with_the_device_solve(gpu_ctx, tmp_path, case):
    from oak_amd.search import forest_search
    from test_gpu_search_forest import network, roots
    if case == "ucb poke-engine":
        n, iterations, kw, net = 96, 48, dict(c=1.0, evaluator="poke-engine"), None
    else:
        net = network(gpu_ctx, tmp_path, "tiny")
        n, iterations, kw = 33, 24, dict(c=1.0, bandit="pucb", evaluator=net)
    b, d, r, seeds, _ = roots(n)
    want = forest_search(gpu_ctx, b, d, r, seeds, iterations, solve_nash=True, **kw)
    got = forest_search(gpu_ctx, b, d, r, seeds, iterations, solve_nash="device", **kw)
    same_trees(got, want)
    assert sum(1 for t in want if abs(sum(t["raw"].p1_nash) - 1.0) < 1e-9) == n             # the strategies are there to compare
    off = forest_search(gpu_ctx, b, d, r, seeds, iterations, solve_nash=False, **kw)
    assert all(not any(t["raw"].p1_nash) and t["raw"].nash_value == 0.0 for t in off)
    if net is not None:
        net.close()


def test_kept_forest_search_with_the_device_solve(gpu_ctx):
    from oak_amd.search import Forest, forest_search
    from test_gpu_search_forest import roots
    b, d, r, seeds, _ = roots(33)
    out = {}
    for mode in (True, "device"):
        forest = Forest(gpu_ctx, 33, 16, keep_arena=0)
        first = forest_search(gpu_ctx, b, d, r, seeds, 16, c=1.0, evaluator="poke-engine", solve_nash=mode, forest=forest, keep=True)
        again = forest_search(gpu_ctx, b, d, r, seeds + np.uint64(5), 16, c=1.0, evaluator="poke-engine", solve_nash=mode, forest=forest, keep=True)   # the kept trees go on
        forest.close()
        out[mode] = (first, again)
    same_trees(out["device"][0], out[True][0])
    same_trees(out["device"][1], out[True][1])


# ---- 4. self-play ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("evaluator, n, iterations, mode, keep", [("poke-engine", 12, 16, "e0.5-n0.5", False), ("poke-engine", 12, 16, "n", True),
                                                                  ("tiny", 5, 8, "n", False), ("tiny", 5, 8, "e0.5-n0.5", True)])
def test_selfplay_with_the_device_solve(gpu_ctx, tmp_path, evaluator, n, iterations, mode, keep):
    from oak_amd.frames import forest_selfplay, replay_check
    from test_gpu_forest_selfplay import games, network
    teams, battle_seeds, seeds = games(n)
    ev = evaluator if evaluator == "poke-engine" else network(gpu_ctx, tmp_path, evaluator)
    host_stats, dev_stats = {}, {}
    want = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=2.0, evaluator=ev, policy_mode=mode, solve_nash=True, stats=host_stats, keep_node=keep)
    got = forest_selfplay(gpu_ctx, teams, battle_seeds, seeds, iterations, c=2.0, evaluator=ev, policy_mode=mode, solve_nash="device", stats=dev_stats, keep_node=keep)
    assert len(got) == len(want) == (6 if keep else 5)
    assert got[0] == want[0] and all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in range(1, len(want)))
    assert (got[4] == 0).all() and int(got[2].sum()) > n
    rep = replay_check(gpu_ctx, got[0])
    assert len(rep["reports"]) == n and (rep["reports"]["status"] == 0).all() and rep["stopped_at"] == len(got[0])
    turns = host_stats["turns"]
    assert dev_stats["turns"] == turns and dev_stats["rows"] == host_stats["rows"]
    # the host's reads of a call: the live count once a turn (what host_reads has always counted, in both runs), and with the host solve the
    # payoffs down and the strategies up, each with its synchronisation
    assert host_stats["host_reads"] == dev_stats["host_reads"] == turns + 1
    assert (host_stats["loop_syncs"], host_stats["loop_copies"]) == (3 * turns + 1, 3 * turns + 1)
    assert (dev_stats["loop_syncs"], dev_stats["loop_copies"]) == (turns + 1, turns + 1)
    assert dev_stats["loop_syncs"] < host_stats["loop_syncs"] and dev_stats["loop_copies"] < host_stats["loop_copies"]
    if not isinstance(ev, str):
        ev.close()


# ---- 5. matches -----------------------------------------------------------------------------------------------------------------------------------
def test_matches_with_the_device_solve(gpu_ctx):
    from oak_amd.arena import search_games
    from test_gpu_forest_match import LOG, PE8, PE16, openings, same
    from test_gpu_forest_match_records import same_records
    b, d, r, seeds = openings(gpu_ctx, 12)
    seats = (dict(PE16, policy_mode="n"), dict(PE8, policy_mode="e0.5-n0.5"))
    for records in (False, True):
        host_stats, dev_stats = {}, {}
        want = search_games(gpu_ctx, seats, b, d, r, seeds, log_turns=LOG, solve_nash=True, stats=host_stats, records=records)
        got = search_games(gpu_ctx, seats, b, d, r, seeds, log_turns=LOG, solve_nash="device", stats=dev_stats, records=records)
        assert same(got, want) and got["counts"] == want["counts"] and dev_stats == host_stats
        assert int(want["turns"].max()) <= LOG and int(want["turns"].sum()) > 12
        if records:
            same_records(got["records"], want["records"])
            assert len(want["records"][0]["stream"]) > 0
