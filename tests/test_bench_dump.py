"""CPU: what `bench.py --dump-outputs` writes — the marginalised graph and the per-blanket report as float64 .npy files —
must not depend on the order in which the streaming driver completed the blankets (oracle injected as the arithmetic,
emulated device), so that two builds can be compared output for output."""
import os

import numpy as np
import pytest

import bench
from sparsifyposegraph_amd import abi, g2o_io
from sparsifyposegraph_amd.graph import GraphWrapperHIP
from tests import oracle_lib


@pytest.mark.parametrize("budget", [None, 100_000])
def test_dump_outputs_do_not_depend_on_completion_order(budget, tmp_path, monkeypatch):
    if budget:   # a workload whose outputs exceed the budget: a fixed, seeded sample of every array
        monkeypatch.setattr(bench, "DUMP_BYTES", budget)
    ictx = oracle_lib.injected_context()
    g = g2o_io.synth_sphere(2000, 100)
    which = np.array([i for i in range(4, 2000) if i % 2], np.int32)
    for seed in (0, 3):
        hg = GraphWrapperHIP.from_dict(g, ctx=ictx)
        hg.set_stream_emulation(seed)
        hg.marginalizeNoOptimize(which, abi.make_options(6))
        bench.dump_outputs(hg, str(tmp_path / f"seed{seed}"))
    names = sorted(os.listdir(tmp_path / "seed0"))
    assert names == sorted(os.listdir(tmp_path / "seed3"))
    assert {"vertex_ids.npy", "vertex_poses.npy", "edge_data.npy", "blanket_kld.npy"} <= set(names)
    for n in names:
        a, b = np.load(tmp_path / "seed0" / n), np.load(tmp_path / "seed3" / n)
        assert a.dtype == np.float64 and np.isfinite(a).all() and np.array_equal(a, b), n
    if budget:
        assert sum(np.load(tmp_path / "seed0" / n).nbytes for n in names) <= budget
        return
    ids, poses = hg.vertices()
    assert np.array_equal(np.load(tmp_path / "seed3" / "vertex_ids.npy"), ids)
    assert np.array_equal(np.load(tmp_path / "seed3" / "vertex_poses.npy"), poses)
    assert len(np.load(tmp_path / "seed3" / "blanket_root.npy")) == len(which)
