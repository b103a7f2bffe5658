"""The round planner of the HIP backend (csrc/spg_round_plan.hpp: which blanket goes to the persistent worker, to which
bin and kernel variant, to the generic kernel, to the large-blanket pipeline, or to SPG_ECAPACITY) on hand-built round
descriptors. Pure host arithmetic: tests/cpp/plan_demo.cpp is compiled against the planner header and needs no device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")


def test_round_plan_routes(tmp_path):
    exe = str(tmp_path / "plan_demo")
    # (the library only for nfr_ip_pattern_size / nfr_ip_workspace, which size the generic kernel's workspace)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "plan_demo.cpp"),
                           "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan ok" in out.stdout and "FAIL" not in out.stdout
