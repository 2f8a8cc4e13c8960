"""GPU: OakGPU::BuildTrainer (include/oakgpu.hpp) in a child process (tests/cpp_build_trainer_smoke.cc) gives oak_amd.build.Trainer's bytes;
on the CPU the program compiles without a warning and links."""
import os
import subprocess

import numpy as np
import pytest

import build_trainer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(tmp_path):
    exe = str(tmp_path / "cpp_build_trainer_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_build_trainer_smoke.cc"), "-L",
                           os.path.join(ROOT, "oak_amd"), "-loakgpu", "-Wl,-rpath," + os.path.join(ROOT, "oak_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_cpp_face_compiles_and_links(tmp_path):
    _compile(tmp_path)


@pytest.mark.gpu
def test_cpp_face_equals_the_python_face(gpu_ctx, tmp_path):
    from oak_amd import build
    net = R.make_net(4, 33, 5, 7)
    path, out = str(tmp_path / "t.build.net"), str(tmp_path / "out.bin")
    open(path, "wb").write(net)
    run = subprocess.run([_compile(tmp_path), path, out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.endswith("ok\n"), run.stdout + run.stderr
    with build.Trainer(gpu_ctx, net, 4) as tr:
        grads = np.array([0.0, 1e-3, -1.0, 0.5, -2e-5], np.float32)[np.arange(tr.count) % 5]
        for _ in range(3):
            tr.set_gradients(grads)
            tr.adam(1e-2)
            tr.average(0.9)
        m = np.concatenate([x.reshape(-1) for x in tr.read("m").values()])
        want = tr.net_bytes() + tr.net_bytes("average") + m.tobytes()
        assert tr.net_bytes() != net
    assert open(out, "rb").read() == want
