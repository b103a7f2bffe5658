"""tests/cpp/removals_demo.cpp drives selectRemovals of the C++ façade (include/spg_graph_wrapper.hpp) on the GPU and prints
the removals the Python binding returns on the same SE3 graph, bit for bit, in hash order without a forced vertex and in
"oldest" order with one and with max_angle."""
import subprocess

import numpy as np
import pytest

from tests.propose_ref import distance_table
from tests.test_removal_selection import _build_demo


@pytest.mark.gpu
@pytest.mark.parametrize("order,keep,max_angle", [("hash", -1, 0.0), ("oldest", 17, 0.7)])
def test_cpp_facade_removals_match_python(tmp_path, order, keep, max_angle, hip_ctx):
    from sparsifyposegraph_amd import g2o_io
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_sphere(n_poses=200, ring=20)
    path = str(tmp_path / "s200.g2o")
    g2o_io.write_g2o(path, g)
    hg = GraphWrapperHIP.load(path, ctx=hip_ctx)
    ids, poses = hg.vertices()
    assert keep < 0 or keep in ids.tolist()
    radius = float(np.sort(distance_table(6, poses), axis=1)[:, 4].mean())      # the mean distance to the fourth neighbour
    out = subprocess.run([_build_demo(tmp_path), path, repr(radius), repr(max_angle), str(keep), order, str(tmp_path / "cpp.txt")],
                         capture_output=True, text=True)
    assert out.returncode == 0 and "removals ok" in out.stdout, out.stdout + out.stderr
    cpp = np.loadtxt(str(tmp_path / "cpp.txt")).reshape(-1, 3)
    rem, rep, rd = hg.selectRemovals(radius, max_angle, keep=[] if keep < 0 else [keep], priority=None if order == "hash" else order)
    assert len(cpp) == len(rem) > 20
    assert np.array_equal(cpp[:, 0].astype(np.int32), rem) and np.array_equal(cpp[:, 1].astype(np.int32), rep) and np.array_equal(cpp[:, 2], rd)
