"""CPU: the solver text the device runs (oak_amd/csrc/nash.hpp: solve_soft<L> -- the integer simplex on L-limb integers and the x87 long
double roundings restated in integer arithmetic), run on the host through two diagnostic exports, against the host's own long double path
(oakgpu_solve_matrix), bit for bit; against the Fraction simplex of test_search_host.py; and in a stand-alone sanitizer build."""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nash_cases as NC
from test_search_host import solve_matrix_exact
from oak_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _limbs(values):
    """Python ints -> uint64[count, 8], two's complement, least significant limb first"""
    raw = b"".join(int(v).to_bytes(64, "little", signed=True) for v in values)
    return np.frombuffer(raw, dtype="<u8").reshape(len(values), 8).copy()


def _round_both(num, den, shift):
    lib = _lib.load()
    n = len(num)
    a, b, s = _limbs(num), _limbs(den), np.array(shift, dtype=np.int64)
    hard, soft = np.zeros(n), np.zeros(n)
    assert lib.oakgpu_nash_round_host(NC.vp(a), NC.vp(b), NC.vp(s), n, NC.vp(hard), NC.vp(soft)) == 0, lib.oakgpu_last_error()
    return hard, soft


def _random_int(rng, limbs):
    bits = 64 * (limbs - 1) + int(rng.integers(1, 64 if limbs == 8 else 65))
    return int.from_bytes(rng.bytes(64), "little") >> (512 - bits) | 1 << (bits - 1)


def test_rounding_restatement_equals_long_double_on_random_ratios():
    """to_ld / divide / subtract / to double, restated in integers, against the x87 operations themselves: 210,000 ratios of 1- to 8-limb
    integers, a third of them negative, shifts from the solver's range"""
    rng = np.random.default_rng(11)
    shifts = [0, 1, 2, -3, 257, (1 << 20) + 1, -(1 << 20)]
    num, den, shift = [], [], []
    for k in range(210_000):
        a, b = _random_int(rng, 1 + k % 8), _random_int(rng, 1 + (k // 8) % 8)
        num.append(-a if k % 3 == 0 else a)
        den.append(b)
        shift.append(shifts[k % 7])
    hard, soft = _round_both(num, den, shift)
    assert NC.same_bits(hard, soft)
    small = [(int(rng.integers(1, 1 << 40)), int(rng.integers(1, 1 << 40)), int(rng.integers(-(1 << 20), (1 << 20) + 2))) for _ in range(20_000)]
    hard, soft = _round_both([x[0] for x in small], [x[1] for x in small], [x[2] for x in small])   # quotients of the shift's size: the subtraction cancels
    assert NC.same_bits(hard, soft)


def test_rounding_restatement_on_directed_cases():
    rng = np.random.default_rng(12)
    num, den, shift = [], [], []
    for _ in range(500):
        low = int(rng.integers(0, 1 << 63)) * 2 + 1
        num += [(1 << 64) + low, (1 << 64) + low, ((1 << 64) + low) << 64 | 1 << 63, ((1 << 64) + low - 1) << 64 | 1 << 63]
        den += [1, 3, 1, (1 << 64) + low]      # 65 significant bits: a tie when the second limb comes in; a limb of 2^63 below it
        shift += [0, 0, 0, 1]
    for _ in range(500):                       # numerator = denominator; shift 1 and 2^20 + 1 against quotients of their size
        a = _random_int(rng, int(rng.integers(1, 8)))     # (times 2^20 + 1 it still fits eight limbs)
        num += [a, a, a * ((1 << 20) + 1), a * ((1 << 20) + 1) + 1]
        den += [a, a, a, a]
        shift += [0, 1, (1 << 20) + 1, (1 << 20) + 1]
    hard, soft = _round_both(num, den, shift)
    assert NC.same_bits(hard, soft)
    assert hard[4 * 500] == 1.0 and hard[4 * 500 + 1] == 0.0 and hard[4 * 500 + 2] == 0.0
    # double rounding: the exact ratio lies just above a 53-bit midpoint, its 64-bit rounding ON the midpoint, which then goes to even.
    # A correctly rounded double of the exact ratio goes up instead: the restatement must follow the host's two roundings.
    num, den, correct = [], [], []
    for k in range(200):
        top = int(rng.integers(1 << 51, 1 << 52)) * 2 | 1 << 52                 # an even 53-bit mantissa
        exact_num = (top << 18 | 1 << 17) * 3 + 1                              # (top + 1/2 + 1/3 2^-17) 2^18, over 3
        num.append(exact_num)
        den.append(3)
        correct.append(exact_num / 3)                                          # int / int is correctly rounded
    hard, soft = _round_both(num, den, [0] * 200)
    assert NC.same_bits(hard, soft)
    differ = sum(1 for k in range(200) if hard[k] != correct[k])
    assert differ == 200 and all(correct[k] - hard[k] == 2.0 ** 18 for k in range(200))


def _cases():
    # 81 shapes x 250 + 1 = 20,251 matrices
    return NC.batch(21, {"small": 90, "large": 70, "equal": 10, "dup_row": 20, "dup_col": 20, "dominated": 20, "saddle": 20})


@pytest.fixture(scope="module")
def solved():
    lib = _lib.load()
    mats = _cases()
    return mats, NC.host_solve(lib, mats), NC.soft_solve(lib, mats, 8)


def test_solve_soft_8_equals_solve_matrix(solved):
    mats, (p1, p2, v, ok), (q1, q2, u, width) = solved
    assert len(mats) >= 20_000 and ok.all() and (width > 0).all()
    assert {A.shape for A in mats} == {(m, n) for m in range(1, 10) for n in range(1, 10)}
    assert NC.same_bits(p1, q1) and NC.same_bits(p2, q2) and NC.same_bits(v, u)     # the vertex among several equilibria included
    several = sum(1 for k, A in enumerate(mats) if (A == A.flat[0]).all() and A.shape[0] > 1)
    assert several > 500 and set(width.tolist()) == {4, 8}


def test_width_independence_and_the_bound(solved):
    lib = _lib.load()
    mats, _, (q1, q2, u, width) = solved
    narrow = [k for k in range(len(mats)) if width[k] == 4]
    assert len(narrow) > 10_000
    r1, r2, r, w4 = NC.soft_solve(lib, [mats[k] for k in narrow], 4)
    assert NC.same_bits(r1, q1[narrow]) and NC.same_bits(r2, q2[narrow]) and NC.same_bits(r, u[narrow]) and (w4 == 4).all()
    bound = lib.oakgpu_nash_width4_max_entry()         # the largest shifted entry the narrow width takes: from the code
    assert 257 <= bound < 1 << 21
    rng = np.random.default_rng(5)
    at, beyond = [], []
    for _ in range(200):
        m, n = (int(x) for x in rng.integers(1, 10, 2))
        A = rng.integers(0, bound, (m, n))
        A.flat[0], A.flat[-1] = 0, bound - 1           # shifted: 1 ... bound
        at.append(A.copy())
        A.flat[-1] = bound if m * n > 1 else 0         # one step beyond (a 1 x 1 matrix's shifted entry is always 1)
        beyond.append(A)
    a1, a2, av, aw = NC.soft_solve(lib, at, 0)
    b1, b2, bv, bw = NC.soft_solve(lib, beyond, 0)
    assert (aw == 4).all() and all(bw[k] == (8 if beyond[k].size > 1 else 4) for k in range(200))
    for mats2, got in ((at, (a1, a2, av)), (beyond, (b1, b2, bv))):
        w1, w2, wv, _ = NC.soft_solve(lib, mats2, 8)
        h1, h2, hv, ok = NC.host_solve(lib, mats2)
        assert ok.all() and NC.same_bits(got[0], w1) and NC.same_bits(got[1], w2) and NC.same_bits(got[2], wv)
        assert NC.same_bits(h1, w1) and NC.same_bits(h2, w2) and NC.same_bits(hv, wv)


def test_solve_soft_against_the_fraction_simplex():
    """the same vertex as the exact-rational simplex with the same rule.  A strategy is one quotient rounded to 64 bits and then to 53: within
    one unit of the double nearest the exact value.  The value is (v + shift) rounded to 64 bits, minus shift, rounded to 64 and to 53 bits:
    within 2^-63 (|v| + |shift|) + 2^-52 |v| of the exact v."""
    lib = _lib.load()
    mats = NC.batch(33, {"small": 2, "large": 1, "saddle": 1})      # 325 matrices
    assert len(mats) >= 300
    exact = [solve_matrix_exact(A.tolist()) for A in mats]
    for limbs in (0, 8):
        q1, q2, u, width = NC.soft_solve(lib, mats, limbs)
        for k, A in enumerate(mats):
            e1, e2, ev = exact[k]
            m, n = A.shape
            for got, want in ((q1[k, :m], e1), (q2[k, :n], e2)):
                for g, e in zip(got, want):
                    assert abs(g - float(e)) <= np.spacing(float(e)), (k, A.shape)
            shift = 1 - int(A.min())
            assert abs(Fraction(float(u[k])) - ev) <= Fraction(abs(ev) + abs(shift), 1 << 63) + Fraction(abs(ev), 1 << 52), (k, A.shape)
            assert (q1[k, m:] == 0).all() and (q2[k, n:] == 0).all()


def _batch_error(lib, mats_raw, discretize_factor=256):
    """oakgpu_solve_matrices without a context: the refusals come first, they need no device"""
    count = len(mats_raw)
    pay, ms, ns = np.zeros((count, 81), np.int32), np.zeros(count, np.int32), np.zeros(count, np.int32)
    for k, (m, n, values) in enumerate(mats_raw):
        ms[k], ns[k] = m, n
        pay[k, :len(values)] = values
    p1, p2, v = np.zeros((count, 9)), np.zeros((count, 9)), np.zeros(count)
    rc = lib.oakgpu_solve_matrices(None, NC.vp(pay), NC.vp(ms), NC.vp(ns), count, discretize_factor, NC.vp(p1), NC.vp(p2), NC.vp(v))
    return rc, lib.oakgpu_last_error().decode()


def _single_error(lib, m, n, values, discretize_factor=256):
    M = np.zeros(81, np.int32)
    M[:len(values)] = values
    x, y, v = np.zeros(9), np.zeros(9), np.zeros(1)
    rc = lib.oakgpu_solve_matrix(NC.vp(M), m, n, discretize_factor, NC.vp(x), NC.vp(y), NC.vp(v))
    return rc, lib.oakgpu_last_error().decode()


def test_solve_matrices_refuses_what_solve_matrix_refuses():
    lib = _lib.load()
    good = (2, 2, [256, 0, 0, 256])
    cases = [(0, 3, []), (3, 0, []), (10, 1, [0] * 10), (1, 10, [0] * 10), (-1, 2, []), (2, 2, [0, 0, 0, (1 << 20) + 1]), (2, 2, [-(1 << 20) - 1, 0, 0, 0]),
             (2, 2, [0, 0, 0, 1 << 20]), (2, 2, [-(1 << 20), 0, 0, 5]), (9, 9, [7] * 81), (1, 1, [0])]
    for case in cases:
        rc1, msg1 = _single_error(lib, *case)
        rc, msg = _batch_error(lib, [good, good, case, good])
        if rc1 == 0:                       # accepted: the batch goes on to ask for its context
            assert rc != 0 and msg == "oakgpu_solve_matrices: null context", (case[:2], msg)
        else:
            assert rc != 0 and msg == "oakgpu_solve_matrices: matrix 2: " + msg1.split(": ", 1)[1], (case[:2], msg, msg1)
    for factor in (0, -5):
        rc1, msg1 = _single_error(lib, *good, discretize_factor=factor)
        rc, msg = _batch_error(lib, [good], discretize_factor=factor)
        assert rc1 != 0 and rc != 0 and msg.split(": ", 1)[1] == msg1.split(": ", 1)[1]
    rc, msg = _batch_error(lib, [cases[5], cases[0]])
    assert rc != 0 and msg.startswith("oakgpu_solve_matrices: matrix 0: ")      # the lowest refused matrix is named


def test_standalone_program_under_sanitizers(tmp_path):
    """tests/cpp_nash_soft_check.cc (its own main, nothing of Python's in the process): solve_soft at both widths and the rounding
    restatement over the directed families, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "nash_soft_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cpp_nash_soft_check.cc"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-2000:] + run.stderr[-2000:]
