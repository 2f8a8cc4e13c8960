"""CPU: the ABI of the forest search -- liboakgpu.so exports it, oak_amd/_lib.py mirrors its structs byte for byte, the C++ face
(include/oakgpu.hpp: OakGPU::SearchForest) compiles, and every refusal of the contract (include/oakgpu.h) returns its message from the
host-only check both searches run before anything is launched.  No compute call is made."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("oakgpu_forest_create", "oakgpu_forest_destroy", "oakgpu_forest_check", "oakgpu_forest_search_dev", "oakgpu_forest_search",
         "oakgpu_forest_nodes", "oakgpu_forest_last_stats")


def test_library_exports_the_forest_calls():
    import __graft_entry__ as g
    g.build()
    from oak_amd import _lib
    lib = _lib.load()
    for name in CALLS:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None, name


def test_struct_mirrors_have_the_headers_sizes(tmp_path):
    from oak_amd import _lib
    from oak_amd.search import trace_dtype
    src, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "oakgpu.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                         "sizeof(oakgpu_forest_outputs), sizeof(oakgpu_forest_bandit), sizeof(oakgpu_forest_node), sizeof(oakgpu_forest_trace_head), "
                         "sizeof(oakgpu_forest_trace_level), offsetof(oakgpu_forest_outputs, stream), offsetof(oakgpu_forest_bandit, k), "
                         "offsetof(oakgpu_forest_trace_head, value), offsetof(oakgpu_forest_trace_level, i), (size_t)OAKGPU_FOREST_TRACE_BYTES(7)); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    O, B, N, H, L = _lib.ForestOutputs, _lib.ForestBandit, _lib.ForestNode, _lib.ForestTraceHead, _lib.ForestTraceLevel
    assert got == [C.sizeof(O), C.sizeof(B), C.sizeof(N), C.sizeof(H), C.sizeof(L), O.stream.offset, B.k.offset, H.value.offset, L.i.offset,
                   trace_dtype(7).itemsize]
    assert B.priors.offset == 36 and B.visits.offset == 72 and N.p2.offset == C.sizeof(B) and H.logits.offset == 16


def test_cpp_face_compiles(tmp_path):
    src = str(tmp_path / "face.cc")
    open(src, "w").write('#include "oakgpu.hpp"\n'
                         "std::vector<oakgpu_search_output> run(OakGPU::Context &ctx, OakGPU::Network &net, const std::vector<OakGPU::Leaf> &roots,\n"
                         "                                      const std::vector<uint64_t> &seeds) {\n"
                         "  OakGPU::SearchForest forest{ctx, 64, 128, true};\n"
                         "  oakgpu_search_params p = OAKGPU_SEARCH_PARAMS_INIT;\n  p.iterations = 128;\n  p.bandit = 1;\n  p.eval = 1;\n  p.ucb_c = 1.0f;\n"
                         "  std::vector<oakgpu_search_output> out = forest.search(p, roots, seeds, &net, true);\n"
                         "  std::vector<oakgpu_forest_node> nodes = forest.nodes(0, 0, 1);\n"
                         "  return nodes.empty() ? std::vector<oakgpu_search_output>{} : out;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src])


def _check(lib, _lib, max_trees=8, max_iterations=64, contextual=0, has_net=0, n=4, results=None, has_trace=0, trace_levels=0, **fields):
    base = dict(iterations=32, batch=1, ucb_c=1.0, bandit=0, eval=0, max_depth=0, root_rolls=3, other_rolls=1, seed=0, matrix_ucb=0, mucb_delay=0,
                mucb_minimum=0, mucb_c=0.0, exp3_alpha=-1.0, duration_us=0)
    base.update(fields)
    prm = _lib.SearchParams(**base)
    r = np.ascontiguousarray(results, dtype=np.uint8) if results is not None else None
    rc = lib.oakgpu_forest_check(max_trees, max_iterations, contextual, C.byref(prm), has_net, n, r.ctypes.data_as(C.c_void_p) if r is not None else None,
                                 has_trace, trace_levels)
    return rc, lib.oakgpu_last_error().decode()


def test_every_refusal_returns_its_message():
    import __graft_entry__ as g
    g.build()
    from oak_amd import _lib
    lib = _lib.load()
    assert _check(lib, _lib)[0] == 0
    assert _check(lib, _lib, bandit=1, eval=1, contextual=1, has_net=1)[0] == 0
    assert _check(lib, _lib, eval=2, results=[0x50, 0x50, 0x50, 0x50])[0] == 0
    assert _check(lib, _lib, iterations=64, n=8, has_trace=1, trace_levels=100)[0] == 0
    assert _check(lib, _lib, max_depth=3, has_trace=1, trace_levels=3)[0] == 0
    for kwargs, text in ((dict(duration_us=1000), "time budgets are not supported"),
                         (dict(matrix_ucb=1), "matrix_ucb is not supported"),
                         (dict(bandit=2), "the UCB1 bandit is not supported"),
                         (dict(bandit=3), "the Exp3 bandit is not supported"),
                         (dict(bandit=4, eval=1, has_net=1, contextual=1), "the PExp3 bandit is not supported"),
                         (dict(iterations=65), "iterations exceed the forest's max_iterations"),
                         (dict(iterations=0), "give an iteration budget"),
                         (dict(n=9), "n exceeds the forest's max_trees"),
                         (dict(results=[0x50, 0x50, 0x01, 0x50]), "the root position of tree 2 is terminal"),
                         (dict(results=[0x03, 0x50, 0x50, 0x50]), "the root position of tree 0 is terminal"),
                         (dict(has_trace=1, trace_levels=99), "trace_levels must be at least max_depth"),
                         (dict(max_depth=5, has_trace=1, trace_levels=4), "trace_levels must be at least max_depth"),
                         (dict(bandit=1, eval=1, has_net=1, contextual=0), "PUCB needs a forest created contextual"),
                         (dict(bandit=1, eval=0, has_net=1, contextual=1), "PUCB takes its priors from the network evaluator"),
                         (dict(eval=1, has_net=0), "need a network"),
                         (dict(root_rolls=4), "rolls must be 1, 2, 3, 20 or 39")):
        rc, msg = _check(lib, _lib, **kwargs)
        assert rc != 0 and text in msg and msg.startswith("oakgpu_forest_search:"), (kwargs, rc, msg)


def test_the_calls_refuse_null_arguments_without_a_device():
    import __graft_entry__ as g
    g.build()
    from oak_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.oakgpu_forest_create(None, 4, 4, 0, C.byref(h)) != 0 and "oakgpu_forest_create" in lib.oakgpu_last_error().decode()
    prm = _lib.SearchParams(iterations=4, batch=1, root_rolls=3, other_rolls=1)
    assert lib.oakgpu_forest_search(None, None, C.byref(prm), None, None, None, None, 1, None, 0, None, None, 0) != 0
    assert lib.oakgpu_forest_search_dev(None, None, C.byref(prm), None, None, None, None, 1, None, None, 0) != 0
    assert lib.oakgpu_forest_nodes(None, 0, 0, 0, None) != 0
    lib.oakgpu_forest_destroy(None, None)
