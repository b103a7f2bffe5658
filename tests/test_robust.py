"""Robust kernels for optimize() (include/spg.h at spg_graph_set_robust_kernel): g2o's setRobustKernel in IRLS form,
cost = sum rho(s_e), H = sum w_e J^T Omega J, b = -sum w_e J^T Omega e, on the binary edges the kernel applies to.
CPU part: the formulas of tests/robust_ref.py, the setter / getter / clone, and the condition the one-iteration GPU
test rests on. GPU part: per-edge values against the oracle, one LM iteration against the reweighted graph, the fixed
point, outlier rejection, and that nothing outside optimize() sees the kernel."""
import ctypes as C
import functools

import numpy as np
import pytest

from sparsifyposegraph_amd import abi, g2o_io
from tests import oracle_lib, robust_ref
from tests.test_optimize import _perturbed

KIND_NAMES = {robust_ref.HUBER: "huber", robust_ref.CAUCHY: "cauchy", robust_ref.GEMAN_MCCLURE: "geman-mcclure", robust_ref.DCS: "dcs"}
# the graphs of the one-iteration test: the small prefixes of tests/test_optimize.py at its perturbation (sigma = 0.05), and a
# width at which every kind down-weights at least a quarter of the edges while the oracle's LM on the reweighted graph
# still accepts its first trial (test_reweighted_oracle_lm_accepts_its_first_trial checks both)
CASES = [("manhattan_nfr_tree", 150), ("intel_nfr_tree_sp3", 120), ("sphere_nfr_tree", 90)]
SIGMA, DELTA = 0.05, 1.0
# Worst pose difference (max abs over all pose entries) between SPG_SOLVER_DENSE and SPG_SOLVER_SPARSE after one LM iteration
# on the reweighted graphs of CASES x KINDS (weights from numpy and the oracle), measured without this feature in the
# library: the gap between two factorisation orders of one system, which a rounding-level change of that system cannot
# legitimately exceed (the worst was manhattan_nfr_tree with Cauchy). The one-iteration test asserts it.
DENSE_VS_SPARSE_GAP = 2.007283228522283e-13


# ------------------------------------------------------------------------------------------------------- helpers
def _single_edge_chi2(d, kind, ids, data, pose_of):
    """The oracle's chi2 of the graph that holds this edge and its vertices only."""
    og = oracle_lib.OracleGraph(d)
    for v in sorted({int(i) for i in ids}):
        og.L.spgref_graph_add_vertex(og.h, v, oracle_lib._p(np.ascontiguousarray(pose_of[v], np.float64), C.c_double))
    assert og.add_edge(int(kind), ids, data) == 0
    return og.chi2(min(int(i) for i in ids))


def _oracle_edge_chi2(d, ids, poses, edges):
    """Per edge of an edges() dict, at the given estimates."""
    pose_of = {int(i): p for i, p in zip(ids, poses)}
    out = np.zeros(len(edges["kind"]))
    for e in range(len(out)):
        vs = edges["vert_ids"][edges["vert_off"][e]:edges["vert_off"][e + 1]]
        out[e] = _single_edge_chi2(d, edges["kind"][e], vs, edges["data"][edges["data_off"][e]:edges["data_off"][e + 1]], pose_of)
    return out


def _dict_edge_chi2(g):
    """Per edge of a graph dict (binary edges)."""
    pose_of = {int(i): p for i, p in zip(g["ids"], g["poses"])}
    return np.array([_single_edge_chi2(g["pose_dim"], abi.EDGE_BINARY, ij, rec, pose_of) for ij, rec in zip(g["edge_ij"], g["edge_data"])])


def _reweighted(g, w):
    """The same graph with the information of edge e scaled by w[e]."""
    ps = abi.pose_stride(g["pose_dim"])
    data = np.array(g["edge_data"], float).copy()
    data[:, ps:] = w[:, None] * data[:, ps:]
    return dict(g, edge_data=data)


@functools.lru_cache(maxsize=None)
def _case(case, n):
    sub, _, _ = _perturbed(case, n, sigma=SIGMA)
    return sub, _dict_edge_chi2(sub)


def _max_pose_diff(a, b):
    ia, pa = a.vertices()
    ib, pb = b.vertices()
    assert np.array_equal(ia, ib)
    return float(np.abs(pa - pb).max())


# ------------------------------------------------------------------------------------------------------- CPU: formulas
@pytest.mark.parametrize("kind", robust_ref.KINDS)
@pytest.mark.parametrize("delta", [0.5, 1.0, 3.0])
def test_formulas(kind, delta):
    """w = d rho / d s against an mpmath derivative, away from the kinks (Huber: delta^2, DCS: delta). DCS is the one kind
    whose table entries are not a (rho, d rho / d s) pair: with c = 2 Phi / (Phi + s) substituted, c^2 s + Phi (1 - c)^2
    equals Phi for every s > Phi, so its total derivative vanishes there. Its weight c^2 is the derivative with the switch
    variable c held at its current value — how dynamic covariance scaling is defined and what IRLS uses — and that is
    what is checked for it, next to the vanishing total derivative."""
    import mpmath as mp
    mp.mp.dps = 40
    d2 = delta * delta
    dl = mp.mpf(delta)

    def switch(s):
        return min(mp.mpf(1), 2 * dl / (dl + s))

    def rho_mp(s, c=None):
        s = mp.mpf(s)
        if kind == robust_ref.HUBER:
            return s if s <= dl * dl else 2 * dl * mp.sqrt(s) - dl * dl
        if kind == robust_ref.CAUCHY:
            return dl * dl * mp.log1p(s / (dl * dl))
        if kind == robust_ref.GEMAN_MCCLURE:
            return dl * dl * s / (dl * dl + s)
        c = switch(s) if c is None else c
        return c * c * s + dl * (1 - c) ** 2

    grid = [x for x in np.concatenate([np.linspace(0.01, 4.0, 23) * d2, np.linspace(0.013, 5.0, 17) * delta])
            if abs(x - d2) > 1e-3 * d2 and abs(x - delta) > 1e-3 * delta]
    rho, w = robust_ref.rho_w(kind, delta, np.array(grid))
    for s, r, wi in zip(grid, rho, w):
        assert float(abs(rho_mp(s) - mp.mpf(float(r)))) <= 1e-14 * max(1.0, abs(r))
        if kind == robust_ref.DCS:
            c0 = switch(mp.mpf(s))
            assert float(abs(mp.diff(lambda x: rho_mp(x, c0), mp.mpf(s)) - mp.mpf(float(wi)))) <= 1e-13
            total = mp.diff(rho_mp, mp.mpf(s))
            assert float(abs(total - (1 if s < delta else 0))) <= 1e-13
        else:
            assert float(abs(mp.diff(rho_mp, mp.mpf(s)) - mp.mpf(float(wi)))) <= 1e-13
    # rho(0) = 0, w(0) = 1; both continuous across s = delta^2 (and DCS across s = delta)
    r0, w0 = robust_ref.rho_w(kind, delta, np.array([0.0]))
    assert r0[0] == 0.0 and w0[0] == 1.0
    for knee in (d2, delta):
        around = knee * np.array([1 - 1e-9, 1.0, 1 + 1e-9])
        rr, ww = robust_ref.rho_w(kind, delta, around)
        assert np.ptp(rr) <= 1e-8 * knee and np.ptp(ww) <= 1e-8
    if kind == robust_ref.HUBER:
        assert robust_ref.rho_w(kind, delta, np.array([d2]))[1][0] == 1.0
    # concave: the weight never increases, rho stays below its tangent at 0 (the plain s)
    s = np.linspace(0.0, 50.0 * max(d2, delta), 4001)
    rho, w = robust_ref.rho_w(kind, delta, s)
    assert np.all(np.diff(w) <= 1e-15) and np.all(w > 0) and np.all(rho <= s * (1 + 1e-15))
    mid = robust_ref.rho_w(kind, delta, 0.5 * (s[:-1] + s[1:]))[0]
    assert np.all(mid >= 0.5 * (rho[:-1] + rho[1:]) - 1e-13 * np.maximum(1.0, mid))


# ------------------------------------------------------------------------------------------------------- CPU: arguments
@pytest.fixture(scope="module")
def ictx():
    return oracle_lib.injected_context()


def _small(ctx):
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    return GraphWrapperHIP.from_dict(g2o_io.synth_manhattan(40, 8), ctx=ctx)


def test_constants_match_the_reference_module():
    assert (abi.ROBUST_NONE, abi.ROBUST_HUBER, abi.ROBUST_CAUCHY, abi.ROBUST_GEMAN_MCCLURE, abi.ROBUST_DCS) == \
        (robust_ref.NONE, robust_ref.HUBER, robust_ref.CAUCHY, robust_ref.GEMAN_MCCLURE, robust_ref.DCS) == (0, 1, 2, 3, 4)


def test_setter_argument_errors(ictx):
    g = _small(ictx)
    L = g.L
    assert g.robustKernel() == (abi.ROBUST_NONE, 1.0, 1)
    for kind in (-1, 5, 99):
        assert L.spg_graph_set_robust_kernel(g.h, kind, 1.0, 1) == abi.EINVAL
    for delta in (0.0, -1.0, float("nan"), float("inf")):
        assert L.spg_graph_set_robust_kernel(g.h, abi.ROBUST_HUBER, delta, 1) == abi.EINVAL
        assert L.spg_graph_set_robust_kernel(g.h, abi.ROBUST_NONE, delta, 1) == 0     # NONE ignores the width
    assert L.spg_graph_set_robust_kernel(None, abi.ROBUST_HUBER, 1.0, 1) == abi.EINVAL
    assert g.robustKernel()[0] == abi.ROBUST_NONE                                      # a refused call changes nothing
    # refused while a stepwise marginalisation is open
    which = np.array([3, 7], np.int32)
    g.begin(which, abi.make_options(3), 0, 1)
    assert L.spg_graph_set_robust_kernel(g.h, abi.ROBUST_HUBER, 1.0, 1) == abi.EINVAL
    while g.round_prepare() is not None:
        g.round_compute()
        g.round_commit()
    g.end()
    assert L.spg_graph_set_robust_kernel(g.h, abi.ROBUST_HUBER, 1.0, 1) == 0


def test_getter_round_trip_and_gap_clamp(ictx):
    g = _small(ictx)
    for kind in robust_ref.KINDS:
        g.setRobustKernel(kind, 2.5, 3)
        assert g.robustKernel() == (kind, 2.5, 3)
    g.setRobustKernel(abi.ROBUST_CAUCHY, 0.75)
    assert g.robustKernel() == (abi.ROBUST_CAUCHY, 0.75, 1)
    for gap in (0, -4):
        g.setRobustKernel(abi.ROBUST_CAUCHY, 0.75, gap)
        assert g.robustKernel() == (abi.ROBUST_CAUCHY, 0.75, 1)
    g.setRobustKernel(abi.ROBUST_NONE)
    assert g.robustKernel()[0] == abi.ROBUST_NONE
    # every output of the getter may be NULL
    assert g.L.spg_graph_get_robust_kernel(g.h, None, None, None) == 0
    assert g.L.spg_graph_get_robust_kernel(None, None, None, None) == abi.EINVAL


def test_clone_portion_carries_the_setting_and_the_writer_does_not(ictx):
    g = _small(ictx)
    plain = g.writeString()
    g.setRobustKernel(abi.ROBUST_DCS, 1.5, 2)
    c = g.clonePortion(20, optimize=False)
    assert c.robustKernel() == (abi.ROBUST_DCS, 1.5, 2) and c.numVertices() == 21
    assert g.writeString() == plain


def test_edge_chi2_needs_the_hip_backend(ictx):
    g = _small(ictx)
    n = g.numEdges()
    s = np.zeros(n)
    assert g.L.spg_graph_edge_chi2(g.h, None, None, None, 0) == n          # the count is host work
    assert g.L.spg_graph_edge_chi2(g.h, oracle_lib._p(s, C.c_double), None, None, n - 1) == n
    assert g.L.spg_graph_edge_chi2(g.h, oracle_lib._p(s, C.c_double), None, None, n) == abi.ESTATE
    assert g.L.spg_graph_edge_chi2(None, None, None, None, 0) == abi.EINVAL


# ------------------------------------------------------------------------------------------------------- CPU: the condition
@pytest.mark.parametrize("kind", robust_ref.KINDS)
@pytest.mark.parametrize("case,n", CASES)
def test_reweighted_oracle_lm_accepts_its_first_trial(case, n, kind):
    """What test_one_iteration_equals_the_reweighted_graph rests on: with the weights of the start estimates baked into
    the informations, plain LM accepts its first trial — and the kernel really changes the problem."""
    sub, s = _case(case, n)
    fid = int(sub["ids"][0])
    assert s.sum() == pytest.approx(oracle_lib.OracleGraph.from_dict(sub).chi2(fid), rel=1e-12)
    _, w = robust_ref.rho_w(kind, DELTA, s)
    assert np.mean(w < 1) >= 0.25
    st = oracle_lib.OracleGraph.from_dict(_reweighted(sub, w)).optimize(1, fid)
    assert st["trials"] == 1 and st["iterations"] == 1 and st["chi2_final"] < st["chi2_initial"]
    assert st["chi2_initial"] == pytest.approx(float(np.sum(w * s)), rel=1e-12)


# ------------------------------------------------------------------------------------------------------- GPU
def _hip(g, ctx, **kw):
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    return GraphWrapperHIP.from_dict(g, ctx=ctx, **kw)


def _check_edge_values(hg, kind, delta, gap):
    """edgeChi2() of a graph with the kernel set against the oracle (s) and robust_ref on the device's own s (rho, w);
    returns (s, rho, w, eligible)."""
    hg.setRobustKernel(kind, delta, gap)
    ed = hg.edges()
    ids, poses = hg.vertices()
    s, rho, w = hg.edgeChi2()
    ref = _oracle_edge_chi2(hg.d, ids, poses, ed)
    print(f"edge chi2: worst rel {np.max(np.abs(s - ref) / np.maximum(ref, 1e-300)) if len(s) else 0:.2e} over {len(s)} edges")
    assert s == pytest.approx(ref, rel=1e-12)
    nv = np.diff(ed["vert_off"])
    first = ed["vert_ids"][ed["vert_off"][:-1]]
    last = ed["vert_ids"][ed["vert_off"][1:] - 1]
    elig = (ed["kind"] == abi.EDGE_BINARY) & (nv == 2) & (first != last) & (np.abs(first.astype(np.int64) - last) >= max(gap, 1))
    rr, ww = robust_ref.rho_w(kind, delta, s)
    assert rho[elig] == pytest.approx(rr[elig], rel=1e-14) and w[elig] == pytest.approx(ww[elig], rel=1e-14)
    assert np.array_equal(rho[~elig], s[~elig]) and np.all(w[~elig] == 1.0)       # n-ary, exempt and self-loop edges: (s, 1)
    return s, rho, w, elig


@pytest.mark.gpu
@pytest.mark.parametrize("kind", robust_ref.KINDS)
@pytest.mark.parametrize("case,n", CASES)
def test_edge_values_match_oracle_and_formulas(case, n, kind, hip_ctx):
    sub, s_ref = _case(case, n)
    hg = _hip(sub, hip_ctx)
    plain = hg.edgeChi2()                                     # no kernel: (s, s, 1)
    assert np.array_equal(plain[0], plain[1]) and np.all(plain[2] == 1.0)
    s, rho, w, elig = _check_edge_values(hg, kind, DELTA, 1)
    assert elig.all() and np.array_equal(s, plain[0]) and np.mean(w < 1) >= 0.25
    assert s == pytest.approx(s_ref, rel=1e-12)               # edges() keeps the insertion order of the dict
    assert float(s.sum()) == pytest.approx(hg.chi2(), rel=1e-12)
    # min_id_gap = 2 exempts exactly the consecutive-id edges
    s2, rho2, w2, elig2 = _check_edge_values(hg, kind, DELTA, 2)
    consecutive = np.abs(np.diff(np.asarray(sub["edge_ij"], np.int64), axis=1))[:, 0] == 1
    assert np.array_equal(elig2, ~consecutive) and consecutive.any()             # (the intel prefix is one odometry chain)
    assert np.array_equal(w2[elig2], w[elig2]) and np.all(w2[consecutive] == 1.0)


@pytest.mark.gpu
def test_edge_values_nary_self_loop_and_huber_knee(hip_ctx):
    # n-ary GLC edges next to binary ones: a sparsified graph, its estimates perturbed afterwards
    base, which, opts = _perturbed("manhattan_glc_tree", 200, sigma=0.0)
    moved, _, _ = _perturbed("manhattan_glc_tree", 200, sigma=SIGMA)
    hg = _hip(base, hip_ctx, useGLC=True)
    hg.marginalizeNoOptimize(which, opts)
    keep = {int(i) for i in hg.vertices()[0]}
    for i, vid in enumerate(moved["ids"]):
        if int(vid) in keep:
            hg.setEstimate(int(vid), moved["poses"][i])
    kinds = hg.edges()["kind"]
    assert (kinds == abi.EDGE_GLC).any() and (kinds == abi.EDGE_BINARY).any()
    s, rho, w, elig = _check_edge_values(hg, abi.ROBUST_HUBER, 0.5, 1)
    assert np.array_equal(elig, kinds == abi.EDGE_BINARY) and (w[elig] < 1).any()
    assert float(s.sum()) == pytest.approx(hg.chi2(), rel=1e-12)
    # a self-loop and Huber exactly at its knee: Omega = I, pose error (3, 4, 0), delta = 5, so s = delta^2 = 25
    g = _hip({"pose_dim": 3, "ids": np.arange(3, dtype=np.int32), "poses": np.array([[0, 0, 0], [3, 4, 0], [9, 9, 0.5]], float),
              "edge_ij": np.array([[0, 1], [2, 2], [1, 2]], np.int32),
              "edge_data": np.array([[0, 0, 0, 1, 0, 0, 1, 0, 1], [0.5, -0.25, 0.1, 1, 0, 0, 1, 0, 1], [1, 1, 0, 2, 0, 0, 2, 0, 2]], float)}, hip_ctx)
    g.setRobustKernel(abi.ROBUST_HUBER, 5.0)
    s, rho, w = g.edgeChi2()
    assert s[0] == 25.0 and rho[0] == 25.0 and w[0] == 1.0
    assert s[1] == pytest.approx(0.5 ** 2 + 0.25 ** 2 + 0.1 ** 2, rel=1e-12) and rho[1] == s[1] and w[1] == 1.0   # the self-loop is exempt
    assert s[2] > 25.0 and w[2] == pytest.approx(5.0 / np.sqrt(s[2]), rel=1e-14) and rho[2] == pytest.approx(10.0 * np.sqrt(s[2]) - 25.0, rel=1e-14)
    # s = 0 exactly: no division, (0, 0, 1) for every kind
    z = _hip({"pose_dim": 3, "ids": np.arange(2, dtype=np.int32), "poses": np.array([[0, 0, 0], [1, 0, 0]], float),
              "edge_ij": np.array([[0, 1]], np.int32), "edge_data": np.array([[1, 0, 0, 1, 0, 0, 1, 0, 1]], float)}, hip_ctx)
    for kind in robust_ref.KINDS:
        z.setRobustKernel(kind, 0.5)
        assert [float(a[0]) for a in z.edgeChi2()] == [0.0, 0.0, 1.0]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
@pytest.mark.parametrize("ne", [1, 63, 64, 65])
def test_edge_values_around_the_workgroup_size(ne, d, hip_ctx):
    sub, _ = _case("manhattan_nfr_tree", 150) if d == 3 else _case("sphere_nfr_tree", 90)
    ij, data = np.asarray(sub["edge_ij"])[:ne], np.asarray(sub["edge_data"])[:ne]
    used = np.isin(sub["ids"], ij)
    g = dict(sub, ids=np.asarray(sub["ids"])[used], poses=np.asarray(sub["poses"])[used], edge_ij=ij, edge_data=data)
    hg = _hip(g, hip_ctx)
    assert hg.numEdges() == ne
    for kind in (abi.ROBUST_HUBER, abi.ROBUST_DCS):
        s, rho, w, elig = _check_edge_values(hg, kind, 0.5, 1)
        assert len(s) == ne and elig.all()


SOLVERS = [("dense", abi.SOLVER_DENSE), ("sparse", abi.SOLVER_SPARSE), ("pcg", abi.SOLVER_PCG)]


@pytest.fixture(params=SOLVERS, ids=[n for n, _ in SOLVERS])
def solver_ctx(request, hip_ctx):
    hip_ctx.set_linear_solver(request.param[1])
    yield hip_ctx, request.param[1]
    hip_ctx.set_linear_solver(abi.SOLVER_AUTO)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", robust_ref.KINDS)
@pytest.mark.parametrize("case,n", CASES)
def test_one_iteration_equals_the_reweighted_graph(case, n, kind, solver_ctx):
    """Graph A: the kernel, optimize(1). Graph B: no kernel, the informations scaled by the weights A reported before the
    call. The two linear systems are the same numbers, so the poses agree to the gap between two factorisation orders
    (DENSE_VS_SPARSE_GAP); rho is concave, so A accepts the trial B accepts, and A's cost is sum rho where B's is sum w s.
    Measured: the pose difference is exactly 0 for every case, kind and solver."""
    ctx, solver = solver_ctx
    sub, _ = _case(case, n)
    fid = int(sub["ids"][0])
    A = _hip(sub, ctx)
    A.setRobustKernel(kind, DELTA)
    s, rho, w = A.edgeChi2()
    assert np.mean(w < 1) >= 0.25
    B = _hip(_reweighted(sub, w), ctx)
    sa, sb = A.optimize(1, fid), B.optimize(1, fid)
    assert sa["solver"] == solver and sb["solver"] == solver
    assert sa["trials"] == 1 and sb["trials"] == 1 and sa["iterations"] == 1
    assert sa["chi2_initial"] == pytest.approx(float(rho.sum()), rel=1e-12)
    assert sb["chi2_initial"] == pytest.approx(float((w * s).sum()), rel=1e-12)
    diff = _max_pose_diff(A, B)
    print(f"{case} {KIND_NAMES[kind]} solver {solver}: pose difference A - B = {diff:.3e}")
    assert diff <= DENSE_VS_SPARSE_GAP
    # the cost after the step is sum rho at the new estimates
    assert sa["chi2_final"] == pytest.approx(float(A.edgeChi2()[1].sum()), rel=1e-12)
    assert sa["chi2_final"] < sa["chi2_initial"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [robust_ref.HUBER, robust_ref.CAUCHY])
@pytest.mark.parametrize("case,n", [("manhattan_nfr_tree", 150), ("sphere_nfr_tree", 90)])
def test_robust_optimum_is_a_fixed_point_of_the_reweighted_graph(case, n, kind, hip_ctx):
    """At the optimum of sum rho the gradient sum w J^T Omega e vanishes, and that is the gradient of the graph whose
    informations carry the final weights: its own optimize() has nothing to improve (the bound of
    test_oracle_lm_converges_to_a_stationary_point for the same statement)."""
    sub, _ = _case(case, n)
    fid = int(sub["ids"][0])
    A = _hip(sub, hip_ctx)
    A.setRobustKernel(kind, DELTA)
    sa = A.optimize(50, fid)
    s, rho, w = A.edgeChi2()
    assert sa["chi2_final"] < sa["chi2_initial"] and sa["chi2_final"] == pytest.approx(float(rho.sum()), rel=1e-12)
    B = _hip(_reweighted(dict(sub, poses=A.vertices()[1]), w), hip_ctx)
    sb = B.optimize(50, fid)
    print(f"{case} {KIND_NAMES[kind]}: robust cost {sa['chi2_initial']:.6g} -> {sa['chi2_final']:.6g} in {sa['iterations']} it; reweighted "
          f"{sb['chi2_initial']:.12g} -> {sb['chi2_final']:.12g}")
    assert sb["chi2_final"] == pytest.approx(sb["chi2_initial"], rel=1e-9)


def _noise_free(g):
    """The same graph with every measurement taken from the poses (setMeasurementFromState)."""
    data = np.array(g["edge_data"], float).copy()
    for e, (a, b) in enumerate(g["edge_ij"]):
        pa, pb = g["poses"][a], g["poses"][b]
        if g["pose_dim"] == 3:
            c, s = np.cos(pa[2]), np.sin(pa[2])
            dx, dy = pb[0] - pa[0], pb[1] - pa[1]
            data[e, :3] = [c * dx + s * dy, -s * dx + c * dy, (pb[2] - pa[2] + np.pi) % (2 * np.pi) - np.pi]
        else:
            data[e, :3] = g2o_io.quat_rotate(g2o_io.quat_conj(pa[3:]), pb[:3] - pa[:3])
            q = g2o_io.quat_mul(g2o_io.quat_conj(pa[3:]), pb[3:])
            data[e, 3:7] = q if q[3] >= 0 else -q
    return dict(g, edge_data=data)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [robust_ref.CAUCHY, robust_ref.DCS])
@pytest.mark.parametrize("d", [3, 6])
def test_gross_loop_closure_outliers_are_rejected(d, kind, hip_ctx):
    truth = _noise_free(g2o_io.synth_sphere(120, 12) if d == 6 else g2o_io.synth_manhattan(120, 12))
    npos = 3 if d == 6 else 2
    ij = np.asarray(truth["edge_ij"], np.int64)
    odo = np.abs(ij[:, 1] - ij[:, 0]) == 1
    loops = np.nonzero(~odo)[0]
    bad = loops[np.linspace(0, len(loops) - 1, 5).astype(int)]          # 5 loop closures spread over the trajectory
    assert len(set(bad)) == 5
    data = truth["edge_data"].copy()
    data[bad, :npos] += np.array([4.0, -3.0, 2.0])[:npos]
    rng = np.random.default_rng(5)
    P = np.array(truth["poses"], float).copy()
    P[1:, :npos] += 0.02 * rng.standard_normal((len(P) - 1, npos))
    start = dict(truth, edge_data=data, poses=P)

    def worst(h):
        return float(np.linalg.norm(h.vertices()[1][:, :npos] - truth["poses"][:, :npos], axis=1).max())
    plain, robust = _hip(start, hip_ctx), _hip(start, hip_ctx)
    plain.optimize(50, 0)
    robust.setRobustKernel(kind, 1.0, 2)
    robust.optimize(50, 0)
    s, rho, w = robust.edgeChi2()
    clean = ~odo
    clean[bad] = False
    e_plain, e_robust = worst(plain), worst(robust)
    print(f"SE{2 if d == 3 else 3} {KIND_NAMES[kind]}: worst position error plain {e_plain:.3e}, robust {e_robust:.3e}; "
          f"weights corrupted <= {w[bad].max():.3e}, clean loop closures >= {w[clean].min():.3e}")
    assert w[bad].max() < w[clean].min()
    assert np.all(w[odo] == 1.0)
    assert e_robust < e_plain


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", [("manhattan_nfr_tree", 150), ("sphere_nfr_tree", 90)])
def test_nothing_else_moves(case, n, solver_ctx):
    ctx, solver = solver_ctx
    sub, _ = _case(case, n)
    fid = int(sub["ids"][0])
    never = _hip(sub, ctx)
    ref = never.optimize(3, fid)
    # no kernel after set-then-NONE: optimize() is bit-identical to a graph that never had one
    cleared = _hip(sub, ctx)
    cleared.setRobustKernel(abi.ROBUST_CAUCHY, DELTA)
    cleared.setRobustKernel(abi.ROBUST_NONE)
    got = cleared.optimize(3, fid)
    for k in ("iterations", "trials", "chi2_initial", "chi2_final", "lambda_final", "solver"):
        assert got[k] == ref[k], k
    assert np.array_equal(cleared.vertices()[1], never.vertices()[1])
    if solver != abi.SOLVER_DENSE:
        return
    # with a kernel set, everything outside optimize() returns bit for bit what it returns without
    a, b = _hip(sub, ctx), _hip(sub, ctx)
    b.setRobustKernel(abi.ROBUST_CAUCHY, DELTA)
    assert np.array_equal(a.information(fid), b.information(fid))
    for x, y in zip(a.sparseInformation(fid), b.sparseInformation(fid)):
        assert np.array_equal(x, y)
    assert a.chi2() == b.chi2()
    x = np.linspace(-1.0, 1.0, a.d * (a.numVertices() - 1))
    assert np.array_equal(a.informationApply(x, fid), b.informationApply(x, fid))
    assert np.array_equal(a.covariance(fid), b.covariance(fid))
    assert np.array_equal(a.marginalCovariances(fixed_id=fid)[1], b.marginalCovariances(fixed_id=fid)[1])
    # both KLD calls, kernel on the baseline and on the other graph
    _, which, opts = _perturbed(case, n, sigma=SIGMA)
    sa, sb = _hip(sub, ctx), _hip(sub, ctx)
    sb.setRobustKernel(abi.ROBUST_DCS, DELTA)
    sa.marginalizeNoOptimize(which, opts)
    sb.marginalizeNoOptimize(which, opts)
    ea, eb = sa.edges(), sb.edges()
    assert all(np.array_equal(ea[k], eb[k]) for k in ea)
    assert a.kullbackLeibler(sa, fid) == b.kullbackLeibler(sb, fid)
    assert all(a.last_kld_terms[k] == b.last_kld_terms[k] for k in ("kld", "innerprod", "mahalanobis", "logdetx", "logdety"))
    ia, ka = a.marginalKullbackLeibler(sa, fid)
    ib, kb = b.marginalKullbackLeibler(sb, fid)
    assert np.array_equal(ia, ib) and np.array_equal(ka, kb)
    # but optimize() does see it, and chi2(other) with it
    assert b.optimize(3, fid)["chi2_initial"] < ref["chi2_initial"]
