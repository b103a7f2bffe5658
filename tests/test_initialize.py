"""initialize() (spg_graph_initialize, include/spg.h): initial estimates from the measurements alone, by a
breadth-first spanning tree on the host (g2o's computeInitialGuess) or by chordal relaxation on the device
(csrc/spg_init.inc). The checker is tests/chordal_ref.py, a dense numpy restatement of both modes.
CPU part: the reference against first principles (noise-free recovery, the oracle's LM reaches the optimum from it and
not from identity poses) and the host mode / argument checks through an injected backend. GPU part: the device against
the reference, from the four generator graphs down to two vertices."""
import ctypes as C

import numpy as np
import pytest

from sparsifyposegraph_amd import abi, g2o_io
from tests import chordal_ref as ref
from tests import oracle_lib, util

# Device chordal against tests/chordal_ref.py (dense numpy solve and SVD): worst relative pose difference measured on the
# MI355X over every comparison of this file: 8.42e-14, the sparsified manhattan prefix (78 vertices,
# condition numbers 4.8e3 / 6.3e3); the four generator graphs stay below 1.4e-14, the chains of 129 below 5.6e-14. The
# bound is ten times the worst figure, for rounding-order differences between the multifrontal and the dense solve, and
# may never exceed 1e-8.
DEVICE_VS_REFERENCE = 8.42e-13
assert DEVICE_VS_REFERENCE <= 1e-8
# The host spanning tree against the reference: the same compositions in the same order, but libm against numpy for
# cos / sin and differently associated quaternion products — a few ulp per composition, over at most 130 compositions
# on poses of magnitude <= 100: 130 * 4 * 2.2e-16 = 1.2e-13 relative.
TREE_VS_REFERENCE = 1.2e-13

GRAPHS = {
    "sphere_40_8": lambda: g2o_io.synth_sphere(40, 8),
    "sphere_120_12": lambda: g2o_io.synth_sphere(120, 12),
    "manhattan_60_6": lambda: g2o_io.synth_manhattan(60, 6),
    "manhattan_150_10": lambda: g2o_io.synth_manhattan(150, 10),
}
LARGER = ["sphere_120_12", "manhattan_150_10"]


# ------------------------------------------------------------------ small graphs
def _info(d, w):
    diag = np.array([50.0, 30.0, 100.0]) if d == 3 else np.array([10.0, 20.0, 30.0, 400.0, 300.0, 100.0])
    om = np.zeros((d, d))
    om[np.diag_indices(d)] = w * diag
    return om[np.triu_indices(d)]


def _walk(d, n, seed):
    rng = np.random.default_rng(seed)
    P = [np.array([0.3, -0.2, 0.4]) if d == 3 else np.array([0.3, -0.2, 0.1, 0.1, -0.2, 0.3, 0.9])]
    if d == 6:
        P[0][3:] /= np.linalg.norm(P[0][3:])
    for _ in range(n - 1):
        if d == 3:
            step = np.array([1.0, 0.2 * rng.standard_normal(), 0.6 * rng.standard_normal()])
        else:
            q = np.concatenate([0.3 * rng.standard_normal(3), [1.0]])
            step = np.concatenate([[1.0], 0.2 * rng.standard_normal(2), q / np.linalg.norm(q)])
        P.append(ref.compose(d, P[-1], step))
    return np.array(P)


def _graph(d, n, edges, ids=None, seed=0, sigma=0.01):
    """Random-walk ground truth over n vertices; edges = (a, b, weight) by position, (a, b) in the stored direction;
    measurements = the true relative pose with noise of size sigma."""
    rng = np.random.default_rng(1000 + seed)
    P = _walk(d, n, seed)
    ids = np.arange(n, dtype=np.int32) if ids is None else np.asarray(ids, np.int32)
    ij, data = [], []
    for a, b, w in edges:
        z = ref.compose(d, ref.inverse(d, P[a]), P[b])
        if d == 3:
            z = z + sigma * rng.standard_normal(3)
            z[2] = ref.wrap(z[2])
        else:
            dq = np.concatenate([sigma * rng.standard_normal(3), [1.0]])
            z = ref.compose(d, z, np.concatenate([sigma * rng.standard_normal(3), dq / np.linalg.norm(dq)]))
        ij.append((ids[a], ids[b]))
        data.append(np.concatenate([z, _info(d, w)]))
    return {"pose_dim": d, "ids": ids, "poses": P, "edge_ij": np.array(ij, np.int32), "edge_data": np.array(data)}


def _chain(n, closure=True, flip=()):
    e = [((i + 1, i, 1.0) if i in flip else (i, i + 1, 1.0)) for i in range(n - 1)]
    return e + ([(0, n - 1, 2.0)] if closure and n > 2 else [])


# name -> (n, edges, ids, fixed position or -1)
SMALL = {
    "two_forward": (2, [(0, 1, 1.0)], None, -1),
    "two_reverse": (2, [(1, 0, 1.0)], None, -1),
    "triangle": (3, [(0, 1, 1.0), (1, 2, 1.0), (2, 0, 3.0)], None, -1),
    "chain_63": (63, _chain(63), None, -1),
    "chain_64": (64, _chain(64, flip=(5, 40)), None, -1),
    "chain_65": (65, _chain(65), None, -1),
    "chain_129": (129, _chain(129, flip=(1, 2, 77)), None, -1),
    "fixed_last": (65, _chain(65), None, 64),
    "fixed_middle": (66, _chain(66, flip=(30,)), 7 + 3 * np.arange(66), 33),
    "parallel_edges": (6, _chain(6) + [(1, 2, 3.0), (2, 1, 0.5), (4, 3, 7.0)], 100 - 9 * np.arange(6), 2),
}


def _small(d, name):
    n, edges, ids, fpos = SMALL[name]
    g = _graph(d, n, edges, ids, seed=len(name) + d)
    return g, (-1 if fpos < 0 else int(g["ids"][fpos]))


def _by_id(g, poses):
    """poses given in the order of g["ids"] -> ascending id order"""
    return np.asarray(poses)[np.argsort(g["ids"])]


# ------------------------------------------------------------------ CPU: the reference
@pytest.mark.parametrize("name", list(GRAPHS))
def test_reference_recovers_noise_free_ground_truth(name):
    """Measurements rebuilt from the ground truth: both modes return it from identity / zero starts, to 1e-9."""
    g = GRAPHS[name]()
    clean = ref.forget(ref.noise_free(g))
    d = g["pose_dim"]
    got, st = ref.chordal(clean)
    tree, _ = ref.spanning_tree(clean)
    err, terr = ref.pose_diff(got, g["poses"], d), ref.pose_diff(tree, g["poses"], d)
    print(f"{name}: chordal {err:.3g}, tree {terr:.3g}; cond {st['cond_rotation']:.3g} / {st['cond_translation']:.3g}")
    assert st["degenerate"] == 0
    assert err <= 1e-9 and terr <= 1e-9


@pytest.mark.parametrize("name", list(GRAPHS))
def test_oracle_lm_needs_the_initialisation(name):
    """On the noisy graphs the oracle's LM from the reference initialisation reaches the chi2 it reaches from the ground
    truth (1e-9 relative); from identity poses it ends above five times that."""
    g = GRAPHS[name]()
    want = oracle_lib.OracleGraph.from_dict(g).optimize(50, 0)["chi2_final"]
    init, _ = ref.chordal(ref.forget(g))
    got = oracle_lib.OracleGraph.from_dict(dict(g, poses=init)).optimize(50, 0)
    lost = oracle_lib.OracleGraph.from_dict(ref.forget(g)).optimize(50, 0)["chi2_final"]
    print(f"{name}: ground-truth start {want:.9g}, chordal start {got['chi2_final']:.9g} ({got['iterations']:.0f} it), identity start {lost:.6g}")
    assert abs(got["chi2_final"] - want) <= 1e-9 * want
    assert lost > 5 * want


# ------------------------------------------------------------------ CPU: injected backend
@pytest.fixture(scope="module")
def ictx():
    return oracle_lib.injected_context()


def _wrap(g, ctx, forget=True, fixed_id=-1):
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    return GraphWrapperHIP.from_dict(ref.forget(g, fixed_id) if forget else g, ctx=ctx)


def _call(hg, method, fixed_id=-1):
    st = abi.InitStats()
    return hg.L.spg_graph_initialize(hg.h, int(method), int(fixed_id), C.byref(st)), st.asdict()


@pytest.mark.parametrize("d", [3, 6])
@pytest.mark.parametrize("name", list(SMALL))
def test_spanning_tree_matches_reference(d, name, ictx):
    g, fid = _small(d, name)
    hg = _wrap(g, ictx, fixed_id=fid)
    st = hg.initialize(abi.INIT_SPANNING_TREE, fid)
    want, rst = ref.spanning_tree(ref.forget(g, fid), fid)
    err = ref.pose_diff(hg.vertices()[1], _by_id(g, want), d)
    print(f"{name} d={d}: tree depth {st['tree_depth']}, {err:.3g}")
    assert err <= TREE_VS_REFERENCE
    assert (st["method"], st["n_vertices"], st["edges_used"], st["edges_ignored"], st["tree_depth"], st["degenerate"]) == \
        (abi.INIT_SPANNING_TREE, rst["n_vertices"], rst["edges_used"], 0, rst["tree_depth"], 0)
    assert np.isnan(st["chi2_before"]) and np.isnan(st["chi2_after"]) and st["device_seconds"] == 0
    poses = hg.vertices()[1]
    if d == 6:
        assert np.all(poses[:, 6] >= 0) and np.abs(np.linalg.norm(poses[:, 3:], axis=1) - 1).max() <= 4e-16
    else:
        assert np.all(poses[:, 2] > -np.pi) and np.all(poses[:, 2] <= np.pi)


@pytest.mark.parametrize("name", ["sphere_40_8", "manhattan_60_6"])
def test_spanning_tree_on_generator_graphs_and_ignored_edges(name, ictx):
    """The tie-break between two parents of one level (ring closures), a self-loop and a GLC edge that are counted and
    otherwise ignored, and independence of the stored estimates."""
    g = GRAPHS[name]()
    d = g["pose_dim"]
    loop = np.concatenate([g["edge_ij"], [[5, 5]]]), np.concatenate([g["edge_data"], g["edge_data"][:1]])
    g = dict(g, edge_ij=loop[0].astype(np.int32), edge_data=loop[1])
    want, rst = ref.spanning_tree(ref.forget(g))
    results = []
    for forget in (True, False):
        hg = _wrap(g, ictx, forget=forget)
        hg.addGLCEdge([3, 9], np.zeros(2 * d), np.eye(2 * d))
        st = hg.initialize(abi.INIT_SPANNING_TREE)
        results.append(hg.vertices()[1])
        assert (st["edges_used"], st["edges_ignored"], st["tree_depth"]) == (rst["edges_used"], rst["edges_ignored"] + 1, rst["tree_depth"])
        assert rst["edges_ignored"] == 1
    assert ref.pose_diff(results[0], want, d) <= TREE_VS_REFERENCE
    assert np.array_equal(results[0][1:], results[1][1:])


def test_chordal_needs_the_hip_backend(ictx):
    g, _ = _small(3, "triangle")
    hg = _wrap(g, ictx)
    before = hg.vertices()[1].copy()
    rc, _ = _call(hg, abi.INIT_CHORDAL)
    assert rc == abi.ESTATE
    assert np.array_equal(hg.vertices()[1], before)


@pytest.mark.parametrize("d", [3, 6])
def test_argument_errors_leave_the_graph_unchanged(d, ictx):
    g, _ = _small(d, "chain_63")
    hg = _wrap(g, ictx, forget=False)
    before = hg.vertices()[1].copy()

    def refused(method, fixed_id, graph=hg, snapshot=before):
        rc, _ = _call(graph, method, fixed_id)
        assert rc == abi.EINVAL, (method, fixed_id, rc)
        assert np.array_equal(graph.vertices()[1], snapshot)

    for method in (-1, 2, 99):
        refused(method, -1)
    refused(abi.INIT_SPANNING_TREE, 1000)
    assert hg.L.spg_graph_initialize(None, abi.INIT_SPANNING_TREE, -1, None) == abi.EINVAL
    # a vertex whose only link is a GLC edge, and one with no link at all: the message names the smaller id
    hg.addVertex(500, g["poses"][3])
    hg.addVertex(400, g["poses"][4])
    hg.addGLCEdge([7, 400], np.zeros(2 * d), np.eye(2 * d))
    snapshot = hg.vertices()[1].copy()
    refused(abi.INIT_SPANNING_TREE, -1, hg, snapshot)
    assert "vertex 400" in hg.L.spg_last_error(hg.ctx.h).decode()
    refused(abi.INIT_SPANNING_TREE, 400, hg, snapshot)
    # an active stepwise marginalisation
    g2 = _wrap(g, ictx, forget=False)
    g2.begin(np.array([3, 7], np.int32), abi.make_options(d), 0, 1)
    assert _call(g2, abi.INIT_SPANNING_TREE)[0] == abi.EINVAL
    while g2.round_prepare() is not None:
        g2.round_compute()
        g2.round_commit()
    g2.end()
    rc, st = _call(g2, abi.INIT_SPANNING_TREE)
    assert rc == 0 and st["n_vertices"] == 61


@pytest.mark.parametrize("d", [3, 6])
def test_single_vertex_is_a_no_op(d, ictx):
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    hg = GraphWrapperHIP(ctx=ictx, pose_dim=d)
    pose = _walk(d, 1, 0)[0]
    hg.addVertex(12, pose)
    st = hg.initialize(abi.INIT_SPANNING_TREE)
    assert (st["n_vertices"], st["edges_used"], st["edges_ignored"], st["tree_depth"]) == (1, 0, 0, 0)
    assert np.array_equal(hg.vertices()[1][0], pose)
    assert hg.L.spg_graph_initialize(hg.h, abi.INIT_SPANNING_TREE, -1, None) == 0   # the stats are optional


# ------------------------------------------------------------------ GPU
def _device_chordal(g, ctx, fixed_id=-1, forget=True):
    hg = _wrap(g, ctx, forget=forget, fixed_id=fixed_id)
    st = hg.initialize(abi.INIT_CHORDAL, fixed_id)
    return hg, st, hg.vertices()[1]


def _check_against_reference(tag, g, ctx, fixed_id=-1):
    d = g["pose_dim"]
    want, rst = ref.chordal(ref.forget(g, fixed_id), fixed_id)
    hg, st, got = _device_chordal(g, ctx, fixed_id)
    err = ref.pose_diff(got, _by_id(g, want), d)
    print(f"{tag}: device vs reference {err:.3g}; cond {rst['cond_rotation']:.3g} / {rst['cond_translation']:.3g}; chi2 {st['chi2_before']:.6g} -> "
          f"{st['chi2_after']:.6g}; {st['supernodes']} supernodes, {st['device_seconds'] * 1e3:.2f} ms")
    assert err <= DEVICE_VS_REFERENCE
    assert (st["method"], st["n_vertices"], st["edges_used"], st["edges_ignored"], st["tree_depth"], st["degenerate"]) == \
        (abi.INIT_CHORDAL, rst["n_vertices"], rst["edges_used"], rst["edges_ignored"], rst["tree_depth"], rst["degenerate"])
    assert st["chi2_after"] == hg.chi2() and st["supernodes"] >= 1 and st["device_seconds"] > 0
    if d == 6:
        assert np.all(got[:, 6] >= 0) and np.abs(np.linalg.norm(got[:, 3:], axis=1) - 1).max() <= 4e-16
    return hg, st, got


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAPHS))
def test_device_chordal_matches_reference(name, hip_ctx):
    """From identity / zero starts with the noisy measurements."""
    _check_against_reference(name, GRAPHS[name](), hip_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere_120_12", "manhattan_150_10"])
def test_result_does_not_depend_on_the_stored_estimates(name, hip_ctx):
    """Identity, ground truth or random estimates before the call: the same bits after it."""
    g = GRAPHS[name]()
    d = g["pose_dim"]
    rng = np.random.default_rng(5)
    P = np.array(g["poses"], float).copy()
    P[1:] = 10 * rng.standard_normal(P[1:].shape)
    if d == 6:
        P[1:, 3:] /= np.linalg.norm(P[1:, 3:], axis=1, keepdims=True)
    a = _device_chordal(g, hip_ctx, forget=True)[2]
    b = _device_chordal(g, hip_ctx, forget=False)[2]
    c = _device_chordal(dict(g, poses=P), hip_ctx, forget=False)[2]
    assert np.array_equal(a, b) and np.array_equal(a, c)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAPHS))
def test_noise_free_measurements_give_the_ground_truth(name, hip_ctx):
    g = GRAPHS[name]()
    hg, st, got = _device_chordal(ref.noise_free(g), hip_ctx)
    err = ref.pose_diff(got, g["poses"], g["pose_dim"])
    print(f"{name}: {err:.3g}, chi2 {st['chi2_before']:.6g} -> {st['chi2_after']:.3g}")
    assert err <= 1e-9 and st["degenerate"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", LARGER)
def test_initialize_then_optimize_reaches_the_optimum(name, hip_ctx):
    """initialize() then optimize(50) from identity poses against optimize(50) from the ground truth, both on the device."""
    g = GRAPHS[name]()
    want = _wrap(g, hip_ctx, forget=False).optimize(50)
    hg, st, _ = _device_chordal(g, hip_ctx)
    got = hg.optimize(50)
    print(f"{name}: chi2 {st['chi2_before']:.6g} -> initialize {st['chi2_after']:.6g} -> optimize {got['chi2_final']:.9g} in {got['iterations']} it "
          f"(ground-truth start {want['chi2_final']:.9g})")
    assert st["chi2_after"] < st["chi2_before"]
    assert got["chi2_initial"] == st["chi2_after"]
    assert abs(got["chi2_final"] - want["chi2_final"]) <= 1e-9 * want["chi2_final"]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
@pytest.mark.parametrize("name", list(SMALL))
def test_smallest_shapes(d, name, hip_ctx):
    g, fid = _small(d, name)
    _check_against_reference(f"{name} d={d}", g, hip_ctx, fid)


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", [("manhattan_nfr_tree", 150), ("sphere_nfr_tree", 90)])
def test_nfr_tree_result_initialises(case, n, hip_ctx):
    """A graph the device sparsified (NFR Tree: all binary edges, in the library's canonical edge order)."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    gold, which, opts, *_ = util.load_golden(case)
    sub, w = util.prefix_graph(gold, which, n)
    hg = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx)
    hg.marginalizeNoOptimize(w, opts)
    ids, poses = hg.vertices()
    e = hg.edges()
    assert np.all(e["kind"] == abi.EDGE_BINARY)
    g = {"pose_dim": sub["pose_dim"], "ids": ids, "poses": poses, "edge_ij": e["vert_ids"].reshape(-1, 2),
         "edge_data": e["data"].reshape(len(e["kind"]), -1)}
    want, rst = ref.chordal(ref.forget(g))
    for i, p in zip(ids[1:], ref.forget(g)["poses"][1:]):
        hg.setEstimate(int(i), p)
    st = hg.initialize(abi.INIT_CHORDAL)
    err = ref.pose_diff(hg.vertices()[1], want, g["pose_dim"])
    print(f"{case}: {len(ids)} vertices, {len(e['kind'])} edges, device vs reference {err:.3g}, cond {rst['cond_rotation']:.3g} / {rst['cond_translation']:.3g}")
    assert err <= DEVICE_VS_REFERENCE
    assert (st["edges_used"], st["tree_depth"], st["degenerate"]) == (rst["edges_used"], rst["tree_depth"], 0)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_degenerate_vertex_takes_the_tree_orientation(d, hip_ctx):
    """Two parallel edges of equal information whose rotations differ by exactly pi: the relaxed rotation of the free
    vertex vanishes (SE2) / has rank one (SE3); it takes the orientation of the tree — the first edge — and its
    translation is still solved."""
    if d == 3:
        z0, z1 = np.array([1.0, 0.5, 0.0]), np.array([1.25, 0.25, np.pi])
    else:
        z0, z1 = np.array([1.0, 0.5, -0.25, 0, 0, 0, 1.0]), np.array([1.25, 0.25, 0.5, 1.0, 0, 0, 0])
    P = np.array([_walk(d, 1, 0)[0]] * 2)
    g = {"pose_dim": d, "ids": np.array([4, 9], np.int32), "poses": P, "edge_ij": np.array([[4, 9], [4, 9]], np.int32),
         "edge_data": np.array([np.concatenate([z0, _info(d, 1.0)]), np.concatenate([z1, _info(d, 1.0)])])}
    want, rst = ref.chordal(g)
    tree, _ = ref.spanning_tree(g)
    hg, st, got = _device_chordal(g, hip_ctx, forget=False)
    print(f"d={d}: degenerate {st['degenerate']}, pose {got[1]}")
    assert rst["degenerate"] == 1 and st["degenerate"] == 1
    assert ref.pose_diff(got, want, d) <= DEVICE_VS_REFERENCE
    # the orientation is the tree's (the first edge: the fixed vertex's own), the translation the mean of both edges'
    k = 2 if d == 3 else 3
    assert np.abs(got[1][k:] - tree[1][k:]).max() <= TREE_VS_REFERENCE
    assert np.abs(got[1][k:] - P[0][k:]).max() <= TREE_VS_REFERENCE
    R0 = ref.rot2(P[0][2]) if d == 3 else ref.quat_to_R(P[0][3:])
    assert np.abs(got[1][:k] - (P[0][:k] + R0 @ (z0[:k] + z1[:k]) / 2)).max() <= 4e-15


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere_40_8", "manhattan_60_6"])
def test_spanning_tree_on_hip_equals_the_injected_backend(name, hip_ctx, ictx):
    g = GRAPHS[name]()
    a, b = _wrap(g, hip_ctx), _wrap(g, ictx)
    sa, sb = a.initialize(abi.INIT_SPANNING_TREE), b.initialize(abi.INIT_SPANNING_TREE)
    assert np.array_equal(a.vertices()[1], b.vertices()[1])
    drop = ("chi2_before", "chi2_after")
    assert {k: v for k, v in sa.items() if k not in drop} == {k: v for k, v in sb.items() if k not in drop}
    # the device copy moved with the host's: chi2 evaluates on the device
    assert sa["chi2_after"] == a.chi2() != sa["chi2_before"]
    assert a.optimize(50)["chi2_initial"] == sa["chi2_after"]


@pytest.mark.gpu
def test_linear_solver_setting_does_not_apply(hip_ctx):
    g = GRAPHS["sphere_120_12"]()
    auto = _device_chordal(g, hip_ctx)[2]
    for solver in (abi.SOLVER_PCG, abi.SOLVER_DENSE, abi.SOLVER_SPARSE):
        hip_ctx.set_linear_solver(solver)
        try:
            assert np.array_equal(_device_chordal(g, hip_ctx)[2], auto)
        finally:
            hip_ctx.set_linear_solver(abi.SOLVER_AUTO)


@pytest.mark.gpu
def test_nothing_else_moves(hip_ctx):
    """optimize(), kullbackLeibler() and marginalCovariances() of an untouched graph return the same bits before and after
    initialize() ran on a clone."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    from tests.test_optimize import _perturbed
    sub, w, opts = _perturbed("manhattan_nfr_tree", 150, sigma=0.0)
    noisy = _perturbed("manhattan_nfr_tree", 150)[0]
    fid = int(sub["ids"][0])

    def others():
        base, sp = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx), GraphWrapperHIP.from_dict(sub, ctx=hip_ctx)
        sp.marginalizeNoOptimize(w, opts)
        base.kullbackLeibler(sp, fid)
        terms = {k: v for k, v in base.last_kld_terms.items() if k != "device_seconds"}
        hg = GraphWrapperHIP.from_dict(noisy, ctx=hip_ctx)
        st = {k: v for k, v in hg.optimize(50, fid).items() if k != "device_seconds"}
        return terms, base.marginalCovariances(fixed_id=fid)[1], st, hg.vertices()[1]

    before = others()
    untouched = GraphWrapperHIP.from_dict(noisy, ctx=hip_ctx)
    snapshot = untouched.vertices()[1].copy()
    for method in (abi.INIT_CHORDAL, abi.INIT_SPANNING_TREE):
        GraphWrapperHIP.from_dict(noisy, ctx=hip_ctx).initialize(method, fid)
    after = others()
    assert before[0] == after[0] and before[2] == after[2]
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[3], after[3])
    assert np.array_equal(untouched.vertices()[1], snapshot)
