"""CPU: the ABI of the whole-game loop -- liboakgpu.so exports it, oak_amd/_lib.py mirrors its structs byte for byte, and the C++ face
(include/oakgpu.hpp: OakGPU::PolicyGames) compiles.  No compute call is made."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_policy_game_calls():
    import __graft_entry__ as g
    g.build()
    from oak_amd import _lib
    lib = _lib.load()
    for name in ("oakgpu_policy_games_dev", "oakgpu_policy_games"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None, name


def test_struct_mirrors_have_the_headers_sizes(tmp_path):
    from oak_amd import _lib
    src, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "oakgpu.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                         "sizeof(oakgpu_seat), sizeof(oakgpu_policy_games_params), offsetof(oakgpu_seat, net), offsetof(oakgpu_seat, min), "
                         "offsetof(oakgpu_policy_games_params, p2), offsetof(oakgpu_policy_games_params, max_turns), "
                         "offsetof(oakgpu_policy_games_params, log_turns)); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S, P = _lib.Seat, _lib.PolicyGamesParams
    assert got == [C.sizeof(S), C.sizeof(P), S.net.offset, S.min.offset, P.p2.offset, P.max_turns.offset, P.log_turns.offset]
    assert S.kind.offset == 0 and S.temp.offset == S.net.offset + 8 and P.poll.offset == P.max_turns.offset + 4


def test_cpp_face_compiles(tmp_path):
    src = str(tmp_path / "face.cc")
    open(src, "w").write('#include "oakgpu.hpp"\n'
                         "OakGPU::PolicyGames::Result play(OakGPU::Context &ctx, OakGPU::Network &a, OakGPU::Network &b, std::vector<OakGPU::Leaf> &leaves,\n"
                         "                                 std::vector<uint64_t> &rng, const uint8_t *dev, uint8_t *out, uint32_t *turns, float *values) {\n"
                         "  OakGPU::PolicyGames::Params p;\n  p.p1 = &a;\n  p.p2 = &b;\n  p.p1_temp = 0.5;\n  p.log_turns = 8;\n"
                         "  OakGPU::PolicyGames games{ctx, p};\n"
                         "  games.run_dev(dev, dev, dev, out, 1, out, turns, values);\n"
                         "  return games.run(leaves, rng);\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src])
