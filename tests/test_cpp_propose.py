"""tests/cpp/propose_demo.cpp drives proposeCandidates of the C++ façade (include/spg_graph_wrapper.hpp) on the GPU and
prints the pairs the Python binding returns on the same SE3 graph, bit for bit, without and with the range gate."""
import subprocess

import numpy as np
import pytest

from tests.propose_ref import distance_table
from tests.test_candidate_proposal import _build_demo


@pytest.mark.gpu
@pytest.mark.parametrize("rng", [0.0, 1.5])
def test_cpp_facade_proposal_matches_python(tmp_path, rng, hip_ctx):
    from sparsifyposegraph_amd import g2o_io
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_sphere(n_poses=200, ring=20)
    path = str(tmp_path / "s200.g2o")
    g2o_io.write_g2o(path, g)
    hg = GraphWrapperHIP.load(path, ctx=hip_ctx)
    _, poses = hg.vertices()
    radius = float(np.sort(distance_table(6, poses), axis=1)[:, 10].mean())      # the mean distance to the tenth neighbour
    gate = rng * radius / 2.5
    out = subprocess.run([_build_demo(tmp_path), path, repr(radius), "5", "3", repr(gate), str(tmp_path / "cpp.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and "proposal ok" in out.stdout, out.stdout + out.stderr
    cols = 6 if rng > 0 else 4
    cpp = np.loadtxt(str(tmp_path / "cpp.txt")).reshape(-1, cols)
    got = hg.proposeCandidates(radius, min_id_gap=5, max_per_vertex=3, range=gate, z_max=2.0)
    assert len(cpp) == len(got["ij"]) > 50
    assert np.array_equal(cpp[:, :2].astype(np.int32), got["ij"]) and np.array_equal(cpp[:, 2], got["dist"]) and np.array_equal(cpp[:, 3], got["angle"])
    if rng > 0:
        assert np.array_equal(cpp[:, 4], got["sigma"]) and np.array_equal(cpp[:, 5], got["zscore"])
