"""GPU: OakGPU::ReplayWindow (include/oakgpu.hpp) in a child process (tests/cpp_replay_window_smoke.cc) gives oak_amd.train.ReplayWindow's
window, statistics and rows; on the CPU the program compiles without a warning and links."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(tmp_path):
    exe = str(tmp_path / "cpp_replay_window_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_replay_window_smoke.cc"),
                           "-L", os.path.join(ROOT, "oak_amd"), "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_cpp_face_compiles_and_links(tmp_path):
    _compile(tmp_path)


@pytest.mark.gpu
def test_cpp_face_equals_the_python_face(gpu_ctx, tmp_path):
    from oak_amd.train import EncodedBattleFrames, ReplayWindow
    from test_gpu_replay_window import _pool
    pool, _ = _pool(gpu_ctx)
    first, second = b"".join(pool[:3]), b"".join(pool[3:6])
    paths = [str(tmp_path / name) for name in ("first.bin", "second.bin", "out.bin", "saved.battle.data")]
    open(paths[0], "wb").write(first)
    open(paths[1], "wb").write(second)
    run = subprocess.run([_compile(tmp_path)] + paths, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.endswith("ok\n"), run.stdout + run.stderr
    window = ReplayWindow(gpu_ctx, 4, 1 << 30)
    window.append(first)
    st = window.append(second)
    assert st["records"] == 4 and st["evicted"] == 2
    enc = EncodedBattleFrames(33)
    assert window.sample(enc, 77) == 33
    parts = [np.array([st[k] for k in ("records", "bytes", "appended", "evicted", "rejected", "appends")], np.uint64), enc.picks, enc.pokemon, enc.empirical_policies,
             enc.score]
    assert open(paths[2], "rb").read() == b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
    assert open(paths[3], "rb").read() == window.records() == b"".join(pool[2:6])
    window.close()
