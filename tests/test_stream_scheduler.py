"""CPU: the streaming driver's selection rule and commit path (csrc/spg_host_stream.cpp, `Streamer`) — one blanket = one item
handed to the device the moment the rule allows it, committed the moment its result arrives — driven through the C ABI
with the oracle injected as the arithmetic and an EMULATED device that completes the blankets in flight in orders drawn
from a seed (all oldest-first, or random subsets in random order). Whatever the completion order, the result must be
the strictly sequential loop's (src/vertex_remover.cpp:83-140): same vertices, same topology, same payload — and, since
the blanket edges are summed in the reference's sequential edge order (GEdge::key), bit for bit the oracle's numbers.
No GPU, no product arithmetic involved."""
import numpy as np
import pytest

from sparsifyposegraph_amd import abi, g2o_io
from sparsifyposegraph_amd.graph import GraphWrapperHIP
from tests import oracle_lib, util


@pytest.fixture(scope="module")
def ictx():
    return oracle_lib.injected_context()


def _lattice_cases():
    rng = np.random.default_rng(11)
    return {
        "sparsity2": np.array([i for i in range(4, 3000) if i % 2]),
        "random_order": rng.permutation(np.arange(4, 3000))[:1400],       # blankets outgrow the worker: the stream hands over
        "sparsity3": np.array([i for i in range(4, 3000) if i % 3]),         # chains of adjacent removed vertices
        "descending": np.arange(2999, 3, -1)[:1500],
        "every_4th_then_rest": np.concatenate([np.arange(5, 3000, 4), np.arange(7, 3000, 4)]),
    }


@pytest.mark.parametrize("name", list(_lattice_cases()))
@pytest.mark.parametrize("seed", [0, 1, 5])
def test_stream_equals_sequential_on_lattice(name, seed, ictx):
    g = g2o_io.synth_sphere(n_poses=3000, ring=60)
    which = _lattice_cases()[name].astype(np.int32)
    opts = abi.make_options(6)
    og = oracle_lib.OracleGraph.from_dict(g)
    assert og.marginalize(which, opts) == 0
    hg = GraphWrapperHIP.from_dict(g, ctx=ictx)
    hg.set_stream_emulation(seed)
    st = hg.marginalizeNoOptimize(which, opts)
    assert st["n_removed"] == len(which) and st["n_bad_status"] == 0
    ids, _ = hg.vertices()
    oids, _ = og.vertices()
    assert np.array_equal(ids, oids)
    # bit-identical: same blankets, same edge order inside each blanket, same (oracle) arithmetic
    assert util.compare_edge_sets(6, og.edges(), hg.edges(), rtol=0.0) == 0.0
    bl, obl = hg.blankets(), og.blankets()
    o1, o2 = np.argsort(bl["root"], kind="stable"), np.argsort(obl["root"], kind="stable")
    assert np.array_equal(bl["root"][o1], obl["root"][o2])
    assert np.array_equal(bl["status"][o1], obl["status"][o2])
    k1, k2 = bl["kld"][o1], obl["kld"][o2]
    assert np.array_equal(np.isfinite(k1), np.isfinite(k2))
    assert np.array_equal(k1[np.isfinite(k1)], k2[np.isfinite(k2)])


@pytest.mark.parametrize("case", [c for c in util.golden_cases() if "nfr_tree" in c and "local" not in c])
@pytest.mark.parametrize("seed", [0, 3])
def test_stream_on_golden_nfr_tree(case, seed, ictx):
    """The reference's datasets (prefixes + the full-size sphere / parking fixtures): SE2 and SE3, hubs with twenty
    neighbours (parking: the stream hands those blankets to the batch driver), against the committed oracle results."""
    g, which, opts, gold_edges, gold_bl, gold_vids = util.load_golden(case)
    if opts.lin_point != abi.LIN_GLOBAL or opts.topology != abi.TOPO_TREE or opts.algorithm != abi.ALG_NFR:
        pytest.skip("the streaming driver takes NFR Tree at the stored estimates only")
    hg = GraphWrapperHIP.from_dict(g, ctx=ictx)
    hg.set_stream_emulation(seed)
    st = hg.marginalizeNoOptimize(which, opts)
    assert st["n_bad_status"] == 0
    ids, _ = hg.vertices()
    assert np.array_equal(ids, gold_vids)
    util.compare_edge_sets(g["pose_dim"], gold_edges, hg.edges(), rtol=1e-11)


def test_stream_then_more_calls_keep_edge_order(ictx):
    """Two marginalisations and an addEdge in between on one graph: the keys that order a blanket's edges keep following
    the sequential insertion order across calls."""
    g = g2o_io.synth_sphere(n_poses=1200, ring=40)
    opts = abi.make_options(6)
    first = np.array([i for i in range(4, 1200) if i % 4 == 1], np.int32)
    second = np.array([i for i in range(4, 1200) if i % 4 == 3], np.int32)
    og = oracle_lib.OracleGraph.from_dict(g)
    hg = GraphWrapperHIP.from_dict(g, ctx=ictx)
    hg.set_stream_emulation(2)
    assert og.marginalize(first, opts) == 0
    hg.marginalizeNoOptimize(first, opts)
    assert og.marginalize(second, opts) == 0
    st = hg.marginalizeNoOptimize(second, opts)
    assert st["n_bad_status"] == 0
    assert util.compare_edge_sets(6, og.edges(), hg.edges(), rtol=0.0) == 0.0


def test_exposed_edge_order_does_not_depend_on_completion_order(ictx):
    """The stream appends new edges in the order their blankets complete; whatever exposes the edge array (get_edges, the
    .g2o writer, clones, the dense assembly) sees it in key order = the sequential loop's insertion order instead: two runs
    with different completion orders hand out byte-identical arrays and files."""
    g = g2o_io.synth_sphere(n_poses=2000, ring=50)
    which = np.array([i for i in range(4, 2000) if i % 2], np.int32)
    opts = abi.make_options(6)
    outs = []
    for seed in (1, 9):
        hg = GraphWrapperHIP.from_dict(g, ctx=ictx)
        hg.set_stream_emulation(seed)
        hg.marginalizeNoOptimize(which, opts)
        e = hg.edges()
        outs.append((e["kind"].copy(), e["vert_ids"].copy(), e["data"].copy(), hg.writeString()))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert np.array_equal(a, b)
    assert outs[0][3] == outs[1][3]
    # ... and it is the sequential oracle's order
    og = oracle_lib.OracleGraph.from_dict(g)
    assert og.marginalize(which, opts) == 0
    oe = og.edges()
    assert np.array_equal(oe["vert_ids"], outs[0][1]) and np.array_equal(oe["data"], outs[0][2])


# ------------------------------------------------------------------------------------------------- on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("threads", ["1", "0"])
def test_gpu_stream_equals_batch_driver_and_oracle(threads, hip_ctx, monkeypatch):
    """The product on the MI355X: the streaming driver (persistent worker fed one blanket at a time; with and without the
    poll helper thread) against (a) the batch driver on the same device — bit for bit, since both sum a blanket's edges in
    key order and the kernels are the same — and (b) the strictly sequential oracle to the north star's 1e-9."""
    monkeypatch.setenv("SPG_STREAM_THREADS", threads)
    g = g2o_io.synth_sphere(n_poses=20000, ring=200)
    which = np.array([i for i in range(4, 20000) if i % 2], np.int32)
    opts = abi.make_options(6)
    a = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    sa = a.marginalizeNoOptimize(which, opts)
    b = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    b.set_stream_emulation(-2)   # never stream: the batch driver
    sb = b.marginalizeNoOptimize(which, opts)
    assert sa["n_removed"] == sb["n_removed"] == len(which) and sa["n_bad_status"] == sb["n_bad_status"] == 0
    assert sa["n_batches"] > 4 * sb["n_batches"]            # (it did stream: thousands of doorbells against ~200 batches)
    assert util.compare_edge_sets(6, b.edges(), a.edges(), rtol=0.0) == 0.0
    assert sa["kld_sum"] == pytest.approx(sb["kld_sum"], rel=1e-13)
    og = oracle_lib.OracleGraph.from_dict(g)
    assert og.marginalize(which, opts) == 0
    util.compare_edge_sets(6, og.edges(), a.edges(), rtol=util.RTOL)
    kref = float(np.nansum(og.blankets()["kld"]))
    assert abs(kref - sa["kld_sum"]) <= util.RTOL * max(1.0, abs(kref))


@pytest.mark.gpu
def test_gpu_stream_hands_over_on_large_blankets(hip_ctx):
    """parking.g2o (hubs with twenty neighbours): the stream takes what the worker takes, the batch driver the rest; the
    result is the fixture's whatever the split."""
    g, which, opts, gold_edges, gold_bl, gold_vids = util.load_golden("parking_full_nfr_tree")
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    st = hg.marginalizeNoOptimize(np.asarray(which, np.int32), opts)
    assert st["n_bad_status"] == 0 and st["n_removed"] == len(which)
    ids, _ = hg.vertices()
    assert np.array_equal(ids, gold_vids)
    util.compare_edge_sets(6, gold_edges, hg.edges(), rtol=util.RTOL)
