"""Host only: the checks and sizes of kept forests (include/oakgpu.h: oakgpu_forest_create_kept, keep_node in oakgpu_forest_selfplay_check)."""
import os
import re

import numpy as np
import pytest

from oak_amd import _lib
from oak_amd._lib import OakGpuError
from oak_amd.frames import forest_selfplay_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keep_node_needs_a_kept_forest_and_the_refusal_names_its_create():
    ok = dict(max_trees=64, max_iterations=64, contextual=False, iterations=16, n=4)
    with pytest.raises(OakGpuError, match="oakgpu_forest_selfplay: keep_node is not supported.*oakgpu_forest_create_kept"):
        forest_selfplay_check(**dict(ok, keep_node=True))
    forest_selfplay_check(**dict(ok, keep_node=True, kept=True))
    forest_selfplay_check(**dict(ok, kept=True))                                 # a kept forest plays without keep_node too
    forest_selfplay_check(**dict(ok, keep_node=True, kept=True, policy_mode="p", bandit="pucb", evaluator="net", has_net=True, contextual=True))
    with pytest.raises(OakGpuError, match="forest search refuses: PUCB needs a forest created contextual"):   # the kept bit is not `contextual`
        forest_selfplay_check(**dict(ok, keep_node=True, kept=True, bandit="pucb", evaluator="net", has_net=True))
    with pytest.raises(OakGpuError, match="forest search refuses: iterations exceed the forest's max_iterations"):
        forest_selfplay_check(**dict(ok, keep_node=True, kept=True, iterations=65))


def test_keep_arena_below_a_calls_worth_of_nodes_is_refused():
    lib = _lib.load()
    _lib.check(lib.oakgpu_forest_create_kept_check(8, 64, 0))
    _lib.check(lib.oakgpu_forest_create_kept_check(8, 64, 65))
    for arena in (1, 64):
        with pytest.raises(OakGpuError, match="oakgpu_forest_create_kept: keep_arena must be at least max_iterations \\+ 1"):
            _lib.check(lib.oakgpu_forest_create_kept_check(8, 64, arena))
    with pytest.raises(OakGpuError, match="oakgpu_forest_create_kept: max_trees >= 1"):
        _lib.check(lib.oakgpu_forest_create_kept_check(0, 64, 0))
    assert lib.oakgpu_forest_kept_tree_bytes(64, 64) == 0
    with pytest.raises(OakGpuError, match="oakgpu_forest_create_kept: null argument"):
        _lib.check(lib.oakgpu_forest_create_kept(None, 8, 64, 0, 0, None))
    with pytest.raises(OakGpuError, match="oakgpu_forest_advance: null argument"):
        _lib.check(lib.oakgpu_forest_advance_dev(None, None, None, None, None, 0, None))


def test_the_headers_byte_formula_is_what_a_kept_tree_takes():
    """2 * (keep_arena * 224 + slots * 32), slots the power of two >= max(16, 2 * keep_arena): the header's text, restated, against the library."""
    header = open(os.path.join(ROOT, "include", "oakgpu.h")).read()
    text = re.search(r"\n \*\s+(2 \* \(keep_arena \* 224 \+ slots \* 32\)) bytes", header)
    assert text, "the header states the bytes per tree"
    assert "power of two >= max(16, 2 * keep_arena)" in header and "0 = 4 * max_iterations + 1" in header
    lib = _lib.load()
    node, slot = np.dtype([("scores", "<f4", 9), ("priors", "<f4", 9), ("visits", "<u4", 9), ("k", "u1"), ("pad", "u1", 3)]), -(-(8 + 8 + 4 + 4 + 1 + 1 + 2) // 8) * 8
    assert 2 * node.itemsize == 224 == _lib.C.sizeof(_lib.ForestNode) and slot == 32           # (two u64, two u32, i, j, a u16 stamp, padded to 8)
    for iterations, arena in ((1, 0), (1, 2), (7, 0), (8, 9), (16, 17), (256, 0), (256, 257), (256, 2048), (256, 2049), (1000, 4097), (1 << 20, 0)):
        keep_arena = arena if arena else 4 * iterations + 1
        slots = 16
        while slots < 2 * keep_arena:
            slots *= 2
        assert lib.oakgpu_forest_kept_tree_bytes(iterations, arena) == eval(text.group(1), {"keep_arena": keep_arena, "slots": slots}), (iterations, arena)
