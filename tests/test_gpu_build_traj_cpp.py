"""GPU: OakGPU::BuildTrajectories (include/oakgpu.hpp) in a child process (tests/cpp_build_traj_smoke.cc) gives oak_amd.build's arrays; on
the CPU the program compiles without a warning and links."""
import os
import subprocess

import numpy as np
import pytest

import build_traj_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(tmp_path):
    exe = str(tmp_path / "cpp_build_traj_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_build_traj_smoke.cc"), "-L",
                           os.path.join(ROOT, "oak_amd"), "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_cpp_face_compiles_and_links(tmp_path):
    _compile(tmp_path)


@pytest.mark.gpu
def test_cpp_face_equals_the_python_face(gpu_ctx, tmp_path):
    from oak_amd import build
    records = np.concatenate([T.rollout_records(60, 3), np.stack([r for _, _, r in T.malformed_records()])])
    n = len(records)
    data, out = str(tmp_path / "records.bin"), str(tmp_path / "out.bin")
    open(data, "wb").write(records.tobytes())
    run = subprocess.run([_compile(tmp_path), data, out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.endswith("ok\n"), run.stdout + run.stderr
    half = n // 2
    with build.TrajectoryCorpus(gpu_ctx, [records[:half].tobytes(), records[half:].tobytes()]) as corpus:
        want = corpus.decode(np.arange(n, dtype=np.uint32))
        drawn = corpus.sample(33, 77, mask=False, no_score=True)
    t = build.targets(gpu_ctx, want, 0.25)
    parts = [want["action"], want["mask"], want["policy"], want["status"], drawn["picks"], drawn["score"], t["rows"], t["state_cells"], t["old_logp"], t["rewards"]]
    assert open(out, "rb").read() == b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
