"""tests/cpp/robust_demo.cpp: the robust-kernel members of the C++ façade (include/spg_graph_wrapper.hpp: setRobustKernel /
robustKernel / edgeChi2) compile against the C ABI and run on the device."""
import os
import subprocess

import pytest

from sparsifyposegraph_amd import g2o_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")


def _build_demo(tmp_path):
    exe = str(tmp_path / "robust_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "robust_demo.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_robust_demo_compiles(tmp_path):
    out = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr


@pytest.mark.gpu
def test_cpp_facade_robust_kernel(tmp_path):
    path = str(tmp_path / "s200.g2o")
    g2o_io.write_g2o(path, g2o_io.synth_sphere(n_poses=200, ring=20))
    out = subprocess.run([_build_demo(tmp_path), path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "robust ok" in out.stdout
