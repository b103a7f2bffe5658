"""tests/cpp/initialize_demo.cpp: initialize() of the C++ façade (include/spg_graph_wrapper.hpp) compiles against the C ABI
and runs on the device, in both modes, on an SE3 and an SE2 graph."""
import os
import subprocess

import pytest

from sparsifyposegraph_amd import g2o_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")


def _build_demo(tmp_path):
    exe = str(tmp_path / "initialize_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "initialize_demo.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_initialize_demo_compiles(tmp_path):
    out = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr


@pytest.mark.gpu
def test_cpp_facade_initialize(tmp_path):
    exe = _build_demo(tmp_path)
    for name, g in (("s200.g2o", g2o_io.synth_sphere(n_poses=200, ring=20)), ("m150.g2o", g2o_io.synth_manhattan(150, 10))):
        path = str(tmp_path / name)
        g2o_io.write_g2o(path, g)
        out = subprocess.run([exe, path], capture_output=True, text=True)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "initialize ok" in out.stdout
