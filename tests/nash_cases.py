"""Payoff matrices for the Nash solver's tests (test_nash_soft.py on the CPU, test_gpu_device_nash.py on the GPU): every shape 1x1 ... 9x9
with entries from {0 ... 256}, from +-2^20, and from the degenerate families in which the vertex the pivoting rule picks among several
equilibria matters -- all equal, duplicated rows or columns, a dominated row, a saddle point, rock-paper-scissors padded to 9 x 9."""
import ctypes as C

import numpy as np

FAMILIES = ("small", "large", "equal", "dup_row", "dup_col", "dominated", "saddle")


def one(rng, family, m, n):
    if family == "small":
        return rng.integers(0, 257, (m, n))
    if family == "large":
        return rng.integers(-(1 << 20), (1 << 20) + 1, (m, n))
    if family == "equal":
        return np.full((m, n), int(rng.integers(0, 257)))
    A = rng.integers(0, 257, (m, n))
    if family == "dup_row" and m > 1:
        A[rng.integers(1, m)] = A[0]
    elif family == "dup_col" and n > 1:
        A[:, rng.integers(1, n)] = A[:, 0]
    elif family == "dominated" and m > 1:
        A[m - 1] = np.maximum(A[0] - 1, 0)
    elif family == "saddle":
        A = rng.integers(0, 100, (m, n))
        i, j = int(rng.integers(0, m)), int(rng.integers(0, n))
        A[i, :] = rng.integers(150, 200, n)     # the saddle's row: nothing below it ...
        A[:, j] = rng.integers(100, 150, m)     # ... its column: nothing above it
        A[i, j] = 150
    return A


def rock_paper_scissors_padded():
    A = np.zeros((9, 9), np.int64)
    for i in range(9):
        for j in range(9):
            A[i, j] = 128 if i % 3 == j % 3 else (256 if (i % 3 + 2) % 3 == j % 3 else 0)
    return A


def batch(seed, per_shape):
    """per_shape = {family: count}: that many matrices of every family at every shape, plus rock-paper-scissors padded to 9 x 9."""
    rng = np.random.default_rng(seed)
    mats = [rock_paper_scissors_padded()]
    for m in range(1, 10):
        for n in range(1, 10):
            for family, count in per_shape.items():
                mats += [one(rng, family, m, n) for _ in range(count)]
    return mats


def pack(mats):
    """The layout oakgpu_solve_matrices / oakgpu_nash_soft_host take: payoffs int32[count, 81], m int32[count], n int32[count]."""
    pay, ms, ns = np.zeros((len(mats), 81), np.int32), np.zeros(len(mats), np.int32), np.zeros(len(mats), np.int32)
    for k, A in enumerate(mats):
        ms[k], ns[k] = A.shape
        pay[k, :A.size] = np.asarray(A, dtype=np.int32).reshape(-1)
    return pay, ms, ns


def pack_rows(mats):
    """The layout of the forest loops' payoff kernel: int32[count, 82], m | n << 8 at index 81."""
    pay, ms, ns = pack(mats)
    rows = np.zeros((len(mats), 82), np.int32)
    rows[:, :81] = pay
    rows[:, 81] = ms | ns << 8
    return rows


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def host_solve(lib, mats, discretize_factor=1):
    """A loop of oakgpu_solve_matrix: (p1 [count, 9], p2 [count, 9], value [count], ok bool[count]); a refused matrix keeps zeros."""
    count = len(mats)
    p1, p2, v, ok = np.zeros((count, 9)), np.zeros((count, 9)), np.zeros(count), np.zeros(count, bool)
    for k, A in enumerate(mats):
        M = np.ascontiguousarray(A, dtype=np.int32)
        x, y, val = np.zeros(9), np.zeros(9), np.zeros(1)
        if lib.oakgpu_solve_matrix(vp(M), M.shape[0], M.shape[1], int(discretize_factor), vp(x), vp(y), vp(val)) == 0:
            p1[k], p2[k], v[k], ok[k] = x, y, val[0], True
    return p1, p2, v, ok


def soft_solve(lib, mats, limbs):
    """oakgpu_nash_soft_host at `limbs` (0: the selector's): (p1, p2, value in payoff units, width uint8[count], 0 = refused)."""
    pay, ms, ns = pack(mats)
    count = len(mats)
    p1, p2, v, width = np.zeros((count, 9)), np.zeros((count, 9)), np.zeros(count), np.zeros(count, np.uint8)
    rc = lib.oakgpu_nash_soft_host(vp(pay), vp(ms), vp(ns), count, int(limbs), vp(p1), vp(p2), vp(v), vp(width))
    assert rc == 0, lib.oakgpu_last_error()
    return p1, p2, v, width


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))
