"""Outlier edges by greedy data snooping (spg_graph_detect_outliers, csrc/spg_sparse.inc: the sp_prune_*_kernel templates
instantiated with OBJ_STAT) against the numpy rule of tests/outlier_ref.py.
CPU: the candidate-space recurrence equals direct refits of the dense linear model (statistics, residuals, the sum
identity), twin edges of a degree-2 vertex, the planted lattice in numpy alone, the GPU lists are decidable, the argument
contract on an injected backend, the chi^2 quantile, the ABI / bindings / header, the C++ demo compiles.
GPU: sequence and values on constructed lists (before and after marginalisation, both gauges, JOINT / LAZY 1 / LAZY
default), round 0 over every binary edge of a graph with its bridges and the redundancy sum, the planted lattice end to
end, the stop rules and sizes, untouched behaviour, the C++ facade.

Bounds (derived, not measured). beta_i = ||J_i||inf^2 1e-9 max|Sigma| + 1e-11 max|C_ii(0)| is the error model of a
covariance block in candidate space of tests/test_candidate_selection.py, and single_i = 1/2 D ||Omega_i|| D beta_i its
bound of one gain. As in tests/test_edge_pruning.py:
    ||dM_i(0)|| <= D ||Omega_i|| beta_i = 2 single_i / D =: m_i
and every earlier conditioning s added B B^T = C_i* K K^T C_*i, a term of the form of C_ii times at most 1 / lambda_min(M*_s):
    dM_i(t) = (t + 1) m_i / min(1, min_{s<t} lambda_min(M*_s)).
The statistic is stat = z^T M^-1 z with z = L^T e. To first order in dM, and exactly in dz, d(stat) = -z^T M^-1 dM M^-1 z +
2 z^T M^-1 dz + dz^T M^-1 dz, so
    bound_i(t) = |z|^2 dM_i(t) / lambda_min(M_i(t))^2 + (2 |z| + dz_i(t)) dz_i(t) / lambda_min(M_i(t))
with |z|, lambda_min of the reference (the last term matters where an edge sits at its measurement, z = 0). dz_i(0) = ||L_i|| 64 eps geom: the error e_i(0) is a few dozen fp64 operations on
numbers no larger than geom = the largest pose or measurement coordinate. Round s then adds B_i,s w_s to e_i. B = X K with
X = C_i*(s) (error D beta_is (s + 1) / min(1, min lambda*): a cross block with its s history terms; beta_is = max(beta_i,
beta_s) since ||J_i|| ||J_s|| and |C_is| are below the larger of the two squares) and K = L* G^-T, w = G^-1 z*: the
relative error of G^-1 is ||dM*|| / lambda_min(M*) to first order, |w| >= |z*| and ||G^-1|| <= lambda_min^-1/2, so K w is
relatively off by rho_s = (2 dM_s(s) / lambda_s + dz_s(s) / |z_s|) / sqrt(lambda_s), and
    dz_i(t + 1) = dz_i(t) + ||L_i|| (D beta_is (s + 1) / min(1, min lambda*) ||K_s|| |w_s| + ||B_i,s|| |w_s| rho_s):
one ||B|| |w|-sized term per earlier round. A margin moves by at most dM_i(t) / lambda_min(M_i(t))^2 (as the pruning's),
a redundancy (a trace of D entries of M(0)) by D m_i.
The lists are decidable when in every round the best candidate leads the second best by 10 times the larger of their two
bounds. A fixture's own edges tie (twin edges of a degree-2 vertex have EQUAL statistics), so no test asserts a sequence
over them. The sequence lists are 40 added edges between far pairs, Omega = BASE / lambda_i I, whose measurement is the
current relative pose composed with a translation offset of length sqrt(target_i / s_i), target_i = TARGET[0] *
TARGET[1]^rank_i for rank_i = 7 i mod 40 < TARGET[2] and the last value beyond: the statistics are spaced by a factor, largest first.
Measured on an MI355X, worst error over its bound (stat, final_stat, final_margin, redundancy; the same figures under JOINT,
LAZY 1 and LAZY default to two digits): 5.9e-7 (intel NFR Tree), 1.0e-9 (sphere NFR Tree), 8.4e-6 (manhattan GLC Tree); 1.5e-7
on the 300 candidates of the 400-pose manhattan graph; round 0 over every binary edge: 4.9e-7 (statistics), 1.1e-8
(margins), 1.7e-8 (redundancies). Smallest lead over 10 bounds: intel 2.2e3, sphere 17.1, manhattan GLC Tree 98.9 (on the
device's graphs), the planted lattice 160.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sparsifyposegraph_amd import abi, chi2, g2o_io, lib
from sparsifyposegraph_amd.lib import SpgError
from tests import oracle_lib, util
from tests import outlier_ref as orf
from tests import prune_ref as pr
from tests import relative_ref as rr
from tests import select_ref as sr
from tests.test_candidate_selection import _at, _oracle_graphs, _poses, _random_problem, _single_bounds, _fids
from tests.test_covariance_blocks import _oracle_of, _small
from tests.test_edge_pruning import CASES, _add_list, _binary_edges, _edge_rows
from tests.test_relative_covariance import _far_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")
_f64p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
EINVAL, ESTATE = -1, -7
BASE = 0.005                 # Omega_i = BASE / lambda_i I: weak edges, so that a rejection moves the other residuals little
TARGET = (400.0, 0.5, 12)    # target_i = 400 * 0.5^min(i, 12)
K, N_ADD = 8, 40
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------- shared helpers
def _rank(i):
    """the place of candidate i in the grading: a permutation of 0 .. 39, so that the sequence is not the index order"""
    return (7 * i) % N_ADD


def _offset_edges(d, view, fid, Sig):
    """The constructed list on a graph view with covariance Sig (both BEFORE the additions): 40 far pairs, Omega_i = s_i I
    with s_i = BASE / lambda_i, lambda_i = tr(C_ii) / D, z = the current relative pose composed with a translation of
    length sqrt(target_i / s_i) along x. Returns (ij, meas, info_upper)."""
    ids = [int(i) for i in view.vertices()[0]]
    poses = _poses(view)
    far = _far_pairs(view, N_ADD, seed=fid)
    rel = np.array([rr.between(d, poses[int(a)], poses[int(b)]) for a, b in far])
    T = sr.terms(d, poses, _at(ids, fid), far, rel, np.tile(rr.upper(np.eye(d)), (N_ADD, 1)))
    meas, info = [], []
    for i, t in enumerate(T):
        idx, J = sr._support(t, d)
        lam = np.trace(J @ Sig[np.ix_(idx, idx)] @ J.T) / d
        s = BASE / lam
        off = np.zeros(d)
        off[0] = np.sqrt(TARGET[0] * TARGET[1] ** min(_rank(i), TARGET[2]) / s)
        meas.append(rr.compose(d, rel[i], rr.from_mqt(off) if d == 6 else off))
        info.append(rr.upper(s * np.eye(d)))
    return far, np.array(meas), np.array(info)


def _problem(d, view, fid, H0):
    """The constructed list, the information H1 with the 40 edges added, its inverse, the candidates' terms and geom"""
    ids = [int(i) for i in view.vertices()[0]]
    ij, meas, info = _offset_edges(d, view, fid, np.linalg.inv(H0))
    poses = _poses(view)
    T = sr.terms(d, poses, _at(ids, fid), ij, meas, info)
    H1 = H0 + sum(t["A"].T @ t["Om"] @ t["A"] for t in T)
    geom = max(1.0, max(float(np.abs(p[:3 if d == 6 else 2]).max()) for p in poses.values()), float(np.abs(meas[:, :3 if d == 6 else 2]).max()))
    return ij, meas, info, T, H1, np.linalg.inv(H1), geom


def _betas(d, T, single):
    """beta_i and m_i of the module docstring from single_i"""
    om = np.array([np.linalg.norm(t["Om"], 2) for t in T])
    m = 2.0 * single / d
    return m / (d * om), m


def _bounds(d, ref, T, single, geom):
    """bound_i(t), margin bound_i(t) for every round of a reference run (and the round after the last): two lists of
    {i: bound}, and min(1, min lambda*) after the last conditioning"""
    beta, m = _betas(d, T, single)
    n = len(T)
    dz = {i: None for i in range(n)}
    out, mout, star = [], [], 1.0
    for t, ev in enumerate(ref["rounds"]):
        for i, v in ev.items():
            if dz[i] is None:
                dz[i] = v[4] * 64 * EPS * geom
        dM = {i: (t + 1) * m[i] / star for i in ev}
        lam = {i: max(v[2], 1e-150) for i, v in ev.items()}
        out.append({i: v[3] ** 2 * dM[i] / lam[i] ** 2 + (2 * v[3] + dz[i]) * dz[i] / lam[i] for i, v in ev.items()})
        mout.append({i: dM[i] / lam[i] ** 2 for i in ev})
        if t < len(ref["flagged"]):
            s = int(ref["flagged"][t])
            nK, nw, nB = ref["conds"][t]
            lam_s, z_s = ev[s][2], ev[s][3]
            rho = (2 * dM[s] / lam_s + dz[s] / max(z_s, 1e-300)) / np.sqrt(lam_s)
            for i, b in nB.items():
                L_i = ev[i][4]
                dz[i] = dz[i] + L_i * (d * max(beta[i], beta[s]) * (t + 1) / star * nK * nw + b * nw * rho)
            star = min(star, lam_s)
    return out, mout, star


def _lead(ref, bounds):
    """smallest (best - second best) / (10 * larger bound) over the rounds of a reference run"""
    worst = np.inf
    for t in range(len(ref["flagged"])):
        ev, best = ref["rounds"][t], int(ref["flagged"][t])
        others = [i for i in ev if i != best and not np.isnan(ev[i][0])]
        if not others:
            continue
        second = max(others, key=lambda i: ev[i][0])
        worst = min(worst, (ev[best][0] - ev[second][0]) / (10.0 * max(bounds[t][best], bounds[t][second])))
    return worst


# ------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("d", [3, 6])
def test_recurrence_equals_direct_refits(d):
    """Random SPD H0 over 8 poses plus 12 candidate edges, k = 6, a prior centred so that x = 0 is the minimiser: the
    candidate-space recurrence and the Woodbury form give the sequence of the direct refits of the dense linear model, every
    round's statistics and updated residuals to 1e-10 (relative), the redundancies, and the sum identity: the flagged
    statistics add up to chi2(0) - chi2 of the refit without the flagged edges."""
    H0, T = _random_problem(d, seed=d)
    c = orf.refit_model(H0, T)
    n = len(T)
    ok = [True] * n
    H = H0 + sum(t["A"].T @ t["Om"] @ t["A"] for t in T)
    x0, chi0, _ = orf.refit(H0, c, T, list(range(n)))
    assert np.abs(x0).max() <= 1e-12 * max(1.0, np.abs(c).max())          # x = 0 is the minimiser
    exact = orf.refit_greedy(H0, c, T, ok, 6)
    assert len(exact["flagged"]) == 6
    Sig = np.linalg.inv(H)
    rec, woo = orf.recurrence(Sig, T, ok, 6), orf.greedy_sigma(Sig, T, ok, 6)
    for other in (rec, woo):
        assert np.array_equal(other["flagged"], exact["flagged"])
        assert np.allclose(other["stat"], exact["stat"], rtol=1e-10, atol=0)
        assert len(other["rounds"]) == len(exact["rounds"]) == 7
        for t, ev in enumerate(exact["rounds"]):
            assert set(ev) == set(other["rounds"][t])
            for i, v in ev.items():
                assert other["rounds"][t][i][0] == pytest.approx(v[0], rel=1e-10), (t, i)
                assert other["rounds"][t][i][1] == pytest.approx(v[1], rel=1e-9), (t, i)
        live = ~np.isnan(exact["final_stat"])
        assert np.array_equal(live, ~np.isnan(other["final_stat"])) and live.sum() == n - 6
        assert np.allclose(other["final_stat"][live], exact["final_stat"][live], rtol=1e-10, atol=0)
        assert np.allclose(other["redundancy"], exact["redundancy"], rtol=1e-10, atol=0)
        assert np.array_equal(other["status"], exact["status"])
    for t, res in enumerate(exact["resid"]):
        for i, e in res.items():
            assert np.allclose(rec["resid"][t][i], e, rtol=1e-10, atol=1e-10 * np.abs(e).max()), (t, i)
    # the sum identity, and each statistic as a chi2 drop
    rest = [j for j in range(n) if j not in exact["flagged"]]
    assert rec["stat"].sum() == pytest.approx(chi0 - orf.refit(H0, c, T, rest)[1], rel=1e-10)
    assert np.allclose(-np.diff(exact["chi2"][:7]), rec["stat"], rtol=1e-10, atol=0)
    assert np.all(exact["redundancy"] >= 0) and np.all(exact["redundancy"] <= d)
    # min_stat between the third and the fourth statistic stops after three
    mid = 0.5 * (exact["stat"][2] + exact["stat"][3])
    if exact["stat"][3] < exact["stat"][2]:
        assert np.array_equal(orf.recurrence(Sig, T, ok, 6, min_stat=mid)["flagged"], exact["flagged"][:3])
    assert len(orf.recurrence(Sig, T, ok, 6, min_stat=2 * exact["stat"][0])["flagged"]) == 0


def _twin_graph():
    """Five SE2 poses: a 4-cycle 0-1-2-3 with a chord 0-2, and vertex 4 hanging between 1 and 3 by exactly two edges"""
    rng = np.random.default_rng(11)
    poses = np.array([[0, 0, 0.1], [1, 0, 0.4], [1, 1, -0.3], [0, 1, 0.2], [0.5, 0.5, 0.0]], np.float64)
    ij = np.array([(0, 1), (1, 2), (2, 3), (3, 0), (0, 2), (1, 4), (4, 3)], np.int32)
    meas = np.array([rr.between(3, poses[a], poses[b]) + 0.05 * rng.normal(size=3) for a, b in ij])
    info = np.array([rr.upper(B @ B.T + np.eye(3)) for B in rng.normal(size=(len(ij), 3, 3))])
    return {"pose_dim": 3, "ids": np.arange(5, dtype=np.int32), "poses": poses, "edge_ij": ij, "edge_data": np.concatenate([meas, info], axis=1)}


def _graph_terms(g, poses=None, fid=None):
    ids = [int(i) for i in g["ids"]]
    fid = ids[0] if fid is None else fid
    poses = g["poses"] if poses is None else poses
    ps = abi.pose_stride(g["pose_dim"])
    T = sr.terms(g["pose_dim"], {v: np.asarray(poses[k]) for k, v in enumerate(ids)}, _at(ids, fid), g["edge_ij"], g["edge_data"][:, :ps],
                 g["edge_data"][:, ps:])
    return T, sum(t["A"].T @ t["Om"] @ t["A"] for t in T)


def test_twin_edges_of_a_degree_two_vertex_tie():
    """The two edges of a vertex with exactly two edges have equal statistics (at the minimiser: the vertex absorbs either
    residual), in the first round and after a rejection elsewhere; which of the two is wrong cannot be told."""
    g = _twin_graph()
    poses, step = orf.gauss_newton(g, g["poses"])
    assert step < 1e-12
    T, H = _graph_terms(g, poses)
    ref = orf.greedy_sigma(np.linalg.inv(H), T, [True] * 7, 1)
    for ev in ref["rounds"][:2]:
        if 5 in ev and 6 in ev:
            assert ev[5][0] == pytest.approx(ev[6][0], rel=1e-8) and ev[5][0] > 0
    assert np.sum([np.isclose(ref["rounds"][0][i][0], ref["rounds"][0][5][0], rtol=1e-8) for i in range(7)]) == 2


PLANT_Q = 0.999


def _planted():
    g, planted = orf.lattice()
    poses, step = orf.gauss_newton(g, g["poses"], iters=50)
    return g, planted, poses, step


def test_planted_lattice_in_numpy():
    """The 6 x 6 SE2 lattice with three planted 20 sigma loop closures (endpoints of degree >= 3, fixed seed), optimised by
    Gauss-Newton here: the greedy rule at the 0.999 quantile flags exactly the planted set and stops by the threshold (fewer
    than k rounds), every round leads by 10 bounds, and the one-shot threshold flags strictly more than the planted set."""
    g, planted, poses, step = _planted()
    assert step < 1e-10 and len(g["edge_ij"]) == 60 and len(planted) == 3
    deg = np.bincount(g["edge_ij"].ravel())
    assert all(deg[a] >= 3 and deg[b] >= 3 and k >= 35 for k in planted for a, b in [g["edge_ij"][k]])
    T, H = _graph_terms(g, poses)
    Sig = np.linalg.inv(H)
    thr = chi2.chi2_quantile(PLANT_Q, 3)
    ok = [True] * len(T)
    ref = orf.greedy_sigma(Sig, T, ok, 10, min_stat=thr)
    assert sorted(ref["flagged"].tolist()) == planted and len(ref["flagged"]) < 10
    best_left = np.nanmax(ref["final_stat"])
    print(f"planted {planted}: flagged {ref['flagged'].tolist()} at {ref['stat']}, best remaining {best_left:.3f} against {thr:.3f}")
    assert best_left < thr
    single = _single_bounds(3, T, Sig)
    bounds, _, _ = _bounds(3, ref, T, single, geom=6.0)
    lead = _lead(ref, bounds)
    print(f"smallest lead / (10 bounds) {lead:.2e}")
    assert lead >= 1.0
    shot = orf.one_shot(Sig, T, ok, thr)
    print(f"one-shot: {len(shot)} edges over the threshold")
    assert set(planted) < set(shot) and len(shot) > len(planted)
    # the redundancies of a graph of binary edges only sum to D (E - V + 1)
    assert ref["redundancy"].sum() == pytest.approx(3 * (60 - 36 + 1), rel=1e-9)


@pytest.mark.parametrize("case,n", CASES)
def test_constructed_lists_are_decidable(case, n):
    """A condition on the inputs of the GPU sequence test: on the oracle's graphs (before and after its own marginalisation,
    both gauges) the rule flags eight edges of the constructed list and every round's lead is at least 10 bounds; the
    recurrence agrees with the Woodbury form on one configuration."""
    sub, graphs, kept = _oracle_graphs(case, n)
    d = sub["pose_dim"]
    worst, checked = np.inf, False
    for og in graphs:
        ids = [int(i) for i in og.vertices()[0]]
        for fid in _fids(ids, kept):
            ij, meas, info, T, H1, Sig1, geom = _problem(d, og, fid, og.information(fid))
            ref = orf.greedy_sigma(Sig1, T, [True] * N_ADD, K)
            single = _single_bounds(d, T, Sig1)
            bounds, _, _ = _bounds(d, ref, T, single, geom)
            lead = _lead(ref, bounds)
            worst = min(worst, lead)
            print(f"{case}[{n}] fixed {fid}: flagged {ref['flagged'].tolist()}, lead / (10 bounds) {lead:.2e}")
            assert len(ref["flagged"]) == K and lead >= 1.0, (case, fid, ref["flagged"], lead)
            assert [_rank(int(i)) for i in ref["flagged"]] == list(range(K))
            if not checked:
                rec = orf.recurrence(Sig1, T, [True] * N_ADD, K)
                assert np.array_equal(rec["flagged"], ref["flagged"]) and np.allclose(rec["stat"], ref["stat"], rtol=1e-8, atol=0)
                checked = True
    print(f"{case}[{n}]: smallest lead / (10 bounds) {worst:.2e}")


def test_chi2_quantile_is_pinned():
    for dof, q, want in ((3, 0.95, 7.8147), (3, 0.999, 16.2662), (6, 0.95, 12.5916), (6, 0.999, 22.4577)):
        assert abs(chi2.chi2_quantile(q, dof) - want) < 5e-5, (dof, q, chi2.chi2_quantile(q, dof))
        assert chi2.chi2_quantile(q, dof) == pytest.approx(orf.chi2_quantile(q, dof), rel=1e-10)
    assert chi2.chi2_quantile(0.5, 2) == pytest.approx(2 * np.log(2), rel=1e-12)       # chi2_2 is exponential
    with pytest.raises(ValueError):
        chi2.chi2_quantile(1.0, 3)


def test_abi_and_bindings_cover_the_detection():
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    L = C.CDLL(lib.LIB_PATH)
    assert "spg_graph_detect_outliers" in lib.SYMBOLS and hasattr(L, "spg_graph_detect_outliers")
    assert (abi.OUTLIER_INLIER, abi.OUTLIER_INFO_NOT_PD, abi.OUTLIER_UNTESTABLE, abi.OUTLIER_FLAGGED) == (0, 1, 2, 3)
    assert (orf.INLIER, orf.INFO_NOT_PD, orf.UNTESTABLE, orf.FLAGGED) == (0, 1, 2, 3)
    assert C.sizeof(abi.OutlierStats) == C.sizeof(abi.CovSolveStats) + 16 == C.sizeof(abi.PruneStats)
    assert set(abi.OutlierStats().asdict()) >= {"rounds", "endpoints", "detect_seconds", "solve_seconds", "device_seconds", "columns"}
    for m in ("detectOutliers", "rejectOutliers"):
        assert callable(getattr(GraphWrapperHIP, m))
    hdr = open(os.path.join(ROOT, "include", "spg.h")).read()
    for text in ("SPG_OUTLIER_UNTESTABLE = 2", "SPG_OUTLIER_FLAGGED = 3", "spg_outlier_stats", "D (E - V + 1)", "NOT DECIDABLE", "TAKEN\n * AS the minimiser"):
        assert text in hdr, text
    wrap = open(os.path.join(ROOT, "include", "spg_graph_wrapper.hpp")).read()
    assert "detectOutliers" in wrap and "rejectOutliers" in wrap and "OutlierResult" in wrap
    stubs = open(os.path.join(ROOT, "tools", "asan_stubs.cpp")).read()
    assert "hip_sparse_detect" in stubs


def test_detect_checks_arguments_before_the_backend():
    """On an injected (CPU) context, exactly as spg_graph_prune_candidates: the size queries answer; k = 0 and n = 0 return
    0; an index out of range, a non-binary edge, an index listed twice, k < 0, an unknown fixed vertex and an active
    stepwise marginalisation are SPG_EINVAL with their word; a call that would compute is SPG_ESTATE; Python raises."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    sub = _small()
    ictx = oracle_lib.injected_context()
    a = GraphWrapperHIP.from_dict(sub, ctx=ictx)
    ne = a.numEdges()
    ids = [int(v) for v in sub["ids"][:3]]
    a.addGLCEdge(ids, np.zeros(3 * 3), np.eye(9))       # edge index ne: not binary
    L = a.L
    idx = np.array([0, 2, 5, 7], np.int32)
    n = len(idx)
    sel, cs, fs, fm, red, status = np.zeros(n, np.int32), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
    f = lambda x: x.ctypes.data_as(_f64p)  # noqa: E731
    i = lambda x: x.ctypes.data_as(_i32p)  # noqa: E731
    err = lambda: L.spg_last_error(ictx.h).decode()  # noqa: E731

    def detect(ix, cnt, k, cap, fid=-1, h=a.h):
        return L.spg_graph_detect_outliers(h, fid, i(ix), cnt, k, 0.0, 0.0, i(sel), f(cs), cap, f(fs), f(fm), f(red), i(status), None)
    assert detect(idx, n, 2, 0) == 2 and detect(idx, n, 2, 1) == 2 and detect(idx, n, 9, 0) == n
    assert L.spg_graph_detect_outliers(a.h, -1, i(idx), n, 3, 0.0, 0.0, None, None, 99, None, None, None, None, None) == 3
    assert detect(idx, n, 0, n) == 0 and detect(idx, 0, 3, n) == 0
    st = abi.OutlierStats()
    assert detect(idx, n, 2, 2) == ESTATE and "HIP backend" in err()
    assert L.spg_graph_detect_outliers(a.h, -1, i(idx), n, n, 0.0, 0.0, i(sel), f(cs), n, None, None, None, None, C.byref(st)) == ESTATE
    for bad, word in ((np.array([0, ne + 1], np.int32), "out of range"), (np.array([0, -1], np.int32), "out of range"),
                      (np.array([0, ne], np.int32), "not a binary edge"), (np.array([3, 3], np.int32), "listed twice")):
        assert detect(bad, 2, 1, 1) == EINVAL and word in err() and "candidate 1" in err() and "spg_graph_detect_outliers" in err(), err()
    assert detect(idx, n, 2, 2, fid=999999) == EINVAL and "fixed vertex" in err()
    assert detect(idx, n, -1, 2) == EINVAL and "negative" in err()
    g, which, opts, *_ = util.load_golden("intel_nfr_tree_sp3")
    sub2, w = util.prefix_graph(g, which, 30)
    b = GraphWrapperHIP.from_dict(sub2, ctx=ictx)
    b.begin(w, opts, 0, 1)
    assert detect(idx, n, 2, 2, h=b.h) == EINVAL and "active" in err()
    with pytest.raises(SpgError, match="HIP backend"):
        a.detectOutliers(idx, 2)
    with pytest.raises(SpgError, match="listed twice"):
        a.detectOutliers([1, 1], 1)
    with pytest.raises(SpgError, match="negative"):
        a.rejectOutliers(idx, -1)
    got = a.detectOutliers(idx, 0, significance=1e-3)
    assert len(got["flagged"]) == 0 and len(got["stat"]) == 0 and got["final_stat"].shape == (n,) and got["redundancy"].shape == (n,)
    assert got["min_stat"] == pytest.approx(16.2662, abs=5e-5)
    got = a.detectOutliers(np.zeros(0, np.int32), 3)
    assert len(got["flagged"]) == 0 and got["final_margin"].shape == (0,) and got["status"].shape == (0,)
    assert a.numEdges() == ne + 1


def _build_demo(tmp_path):
    exe = str(tmp_path / "outlier_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "outlier_demo.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_outlier_demo_compiles(tmp_path):
    out = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr


# ------------------------------------------------------------------------------------------------------- GPU
MODES = (("joint", abi.GREEDY_JOINT, 0), ("lazy 1", abi.GREEDY_LAZY, 1), ("lazy", abi.GREEDY_LAZY, 0))


def _check_against(d, ref, T, single, geom, got, what):
    """flagged, stat, final_stat, final_margin, redundancy and status of a device run against a reference run; returns
    the worst error / bound"""
    r = len(ref["flagged"])
    assert np.array_equal(got["flagged"], ref["flagged"]), (what, got["flagged"], ref["flagged"])
    bounds, mb, _ = _bounds(d, ref, T, single, geom)
    worst = 0.0
    for t in range(r):
        s = int(ref["flagged"][t])
        err, tol = abs(got["stat"][t] - ref["stat"][t]), bounds[t][s]
        worst = max(worst, err / tol)
        print(f"{what}: round {t} candidate {s} stat {got['stat'][t]:.12g} error / bound {err / tol:.2e}")
        assert err <= tol, (what, t, err, tol)
    assert np.array_equal(got["status"], ref["status"]), (what, got["status"], ref["status"])
    live = ~np.isnan(ref["final_stat"])
    assert np.array_equal(live, ~np.isnan(got["final_stat"])), what
    if live.any():
        last = ref["rounds"][r]
        ix = np.flatnonzero(live)
        err = np.array([abs(got["final_stat"][i] - ref["final_stat"][i]) / bounds[r][i] for i in ix])
        merr = np.array([abs(got["final_margin"][i] - ref["final_margin"][i]) / mb[r][i] for i in ix])
        assert all(i in last for i in ix)
        print(f"{what}: final statistics, worst error / bound {err.max():.2e}; final margins {merr.max():.2e}")
        worst = max(worst, float(err.max()), float(merr.max()))
        assert err.max() <= 1.0 and merr.max() <= 1.0, (what, err.max(), merr.max())
    usable = ~np.isnan(ref["redundancy"])
    rerr = np.abs(got["redundancy"][usable] - ref["redundancy"][usable]) / (2 * single[usable])
    print(f"{what}: redundancies, worst error / bound {rerr.max():.2e}")
    assert rerr.max() <= 1.0 and np.array_equal(usable, ~np.isnan(got["redundancy"]))
    return max(worst, float(rerr.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", CASES)
def test_sequence_and_values_on_constructed_lists(case, n, hip_ctx):
    """The 40 constructed edges are added with addEdge and are the candidates, k = 8, before and after the case's
    marginalisation, both gauges, under JOINT, LAZY lookahead 1 and LAZY default: the reference's sequence exactly (the
    same in the three modes), stat[t], final_stat, final_margin and redundancy within their bounds, the statuses, the
    stats of the call and of the context; the added edges are removed again between the gauges."""
    from tests.test_relative_covariance import _small_graphs
    sub, graphs, kept = _small_graphs(case, n, hip_ctx)
    d = sub["pose_dim"]
    worst, lead = 0.0, np.inf
    try:
        for hg, og in graphs:
            ids = [int(i) for i in hg.vertices()[0]]
            for fid in _fids(ids, kept):
                ij, meas, info, T, H1, Sig1, geom = _problem(d, hg, fid, og.information(fid))
                ref = orf.greedy_sigma(Sig1, T, [True] * N_ADD, K)
                single = _single_bounds(d, T, Sig1)
                lead = min(lead, _lead(ref, _bounds(d, ref, T, single, geom)[0]))
                before = _edge_rows(hg.edges())
                idx = _add_list(hg, ij, meas, info)
                seqs = []
                for name, method, look in MODES:
                    hip_ctx.set_greedy_method(method, look)
                    got = hg.detectOutliers(idx, K, fixed_id=fid)
                    what = f"{case}[{n}] {'after' if hg is graphs[1][0] else 'before'} fixed {fid} {name}"
                    worst = max(worst, _check_against(d, ref, T, single, geom, got, what))
                    s, gs = hg.last_covariance_stats, hip_ctx.greedy_stats()
                    # a lazy call's detect_seconds spans the host's work between round 0 and the rounds (a synchronisation,
                    # the strips' allocation), which device_seconds, two event pairs, leaves out: no order between them
                    assert s["rounds"] == K and 0 < s["detect_seconds"] and (method != abi.GREEDY_JOINT or s["detect_seconds"] < s["device_seconds"])
                    assert s["endpoints"] == len({int(v) for v in ij.ravel()} - {fid})
                    assert gs["method"] == method and gs["rounds"] == K
                    seqs.append(got["flagged"].tolist())
                assert seqs[0] == seqs[1] == seqs[2]
                hg.removeEdges(idx)
                assert _edge_rows(hg.edges()) == before
    finally:
        hip_ctx.set_greedy_method(abi.GREEDY_JOINT, 0)
    print(f"{case}[{n}]: worst error / bound {worst:.2e}, smallest lead / (10 bounds) {lead:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", CASES)
def test_round_zero_over_every_binary_edge(case, n, hip_ctx):
    """Candidates: every binary edge of the graph (before and after the marginalisation, first gauge). With min_stat above
    every statistic nothing is flagged and final_stat / final_margin are the round-0 values: statistics, margins and
    redundancies match numpy on inv(information()) within their bounds wherever numpy's margin is >= 1e-4; the UNTESTABLE
    statuses are exactly the edges whose numpy margin is below 1e-6 and, on graphs of binary edges alone, exactly the
    bridges found by connectivity; there the redundancies sum to D (E - V + 1). No sequence is asserted: the edges tie."""
    from tests.test_relative_covariance import _small_graphs
    sub, graphs, kept = _small_graphs(case, n, hip_ctx)
    d, ps = sub["pose_dim"], abi.pose_stride(sub["pose_dim"])
    for hg, og in graphs:
        ids = [int(i) for i in hg.vertices()[0]]
        fid = ids[0]
        idx, ij, data, nary = _binary_edges(hg)
        Sig = np.linalg.inv(og.information(fid))
        poses = _poses(hg)
        T = sr.terms(d, poses, _at(ids, fid), ij, data[:, :ps], data[:, ps:])
        tl = 3 if d == 6 else 2
        geom = max(1.0, max(float(np.abs(p[:tl]).max()) for p in poses.values()), float(np.abs(data[:, :tl]).max()))
        single = _single_bounds(d, T, Sig)
        ref = orf.greedy_sigma(Sig, T, [t["ok"] for t in T], 0)
        got = hg.detectOutliers(idx, 1, min_stat=1e300, fixed_id=fid)
        assert len(got["flagged"]) == 0 and hg.last_covariance_stats["rounds"] == 0
        ref_bridge = ~(ref["final_margin"] >= 1e-6)
        dev_bridge = got["status"] == abi.OUTLIER_UNTESTABLE
        what = f"{case}[{n}] {'after' if hg is graphs[1][0] else 'before'}"
        print(f"{what}: {dev_bridge.sum()} untestable of {len(idx)} edges")
        assert np.array_equal(dev_bridge, ref_bridge) and np.all(got["status"][~dev_bridge] == abi.OUTLIER_INLIER)
        assert np.all(np.isnan(got["final_stat"][dev_bridge]))
        if not nary:
            at = {v: k for k, v in enumerate(ids)}
            assert np.flatnonzero(dev_bridge).tolist() == pr.connectivity_bridges(len(ids), [(at[int(a)], at[int(b)]) for a, b in ij])
        bounds, mb, _ = _bounds(d, ref, T, single, geom)
        sure = np.flatnonzero(ref["final_margin"] >= 1e-4)
        sb, smb = np.array([bounds[0][i] for i in sure]), np.array([mb[0][i] for i in sure])
        se, me = np.abs(got["final_stat"][sure] - ref["final_stat"][sure]), np.abs(got["final_margin"][sure] - ref["final_margin"][sure])
        re_ = np.abs(got["redundancy"] - ref["redundancy"])
        assert np.all(sb > 0) and np.all(smb > 0) and np.all(np.isfinite(se)) and np.all(np.isfinite(me))
        print(f"  statistics: worst error / bound {(se / sb).max():.2e}; margins {(me / smb).max():.2e}; redundancies {(re_ / (2 * single)).max():.2e}")
        assert np.all(se <= sb) and np.all(me <= smb) and np.all(re_ <= 2 * single)
        assert np.all(got["redundancy"] >= -2 * single) and np.all(got["redundancy"] <= d + 2 * single)
        if not nary:
            want = d * (len(idx) - len(ids) + 1)
            assert abs(got["redundancy"].sum() - want) <= 2 * single.sum() + 1e-12 * want, (got["redundancy"].sum(), want)
            print(f"  redundancy sum {got['redundancy'].sum():.9f} against D (E - V + 1) = {want}")


@pytest.mark.gpu
def test_planted_lattice_end_to_end(hip_ctx):
    """addVertex / addEdge of the planted lattice, optimize(50), detectOutliers over every edge with k = 10 at significance
    1e-3: the flagged set equals the planted set and the numpy reference run at the device's read-back estimates; fewer
    than k are flagged; rejectOutliers then leaves numEdges() - 3 edges."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, planted = orf.lattice()
    hg = GraphWrapperHIP(ctx=hip_ctx, pose_dim=3)
    for v, p in zip(g["ids"], g["poses"]):
        hg.addVertex(int(v), p)
    for (a, b), rec in zip(g["edge_ij"], g["edge_data"]):
        hg.addEdge(int(a), int(b), rec[:3], rec[3:])
    hg.optimize(50)
    ne = hg.numEdges()
    idx = np.arange(ne, dtype=np.int32)
    got = hg.detectOutliers(idx, 10, significance=1e-3)
    _, poses = hg.vertices()
    T, H = _graph_terms(g, poses)
    ref = orf.greedy_sigma(np.linalg.inv(H), T, [True] * ne, 10, min_stat=chi2.chi2_quantile(0.999, 3))
    print(f"planted {planted}: device {got['flagged'].tolist()} at {got['stat']}, numpy {ref['flagged'].tolist()} at {ref['stat']}")
    assert sorted(got["flagged"].tolist()) == planted == sorted(ref["flagged"].tolist()) and len(got["flagged"]) < 10
    assert got["flagged"].tolist() == ref["flagged"].tolist()
    assert np.nanmax(got["final_stat"]) < got["min_stat"] == pytest.approx(16.2662, abs=5e-5)
    assert (got["status"] == abi.OUTLIER_FLAGGED).sum() == 3
    out = hg.rejectOutliers(idx, 10, significance=1e-3)
    assert out["flagged"].tolist() == got["flagged"].tolist() and hg.numEdges() == ne - 3


@pytest.mark.gpu
def test_stop_rules_sizes_and_cap_queries(hip_ctx):
    """synth_manhattan(400) with 300 added far-pair edges as candidates (two workgroups of argmax partials), the first
    twelve offset so that the order is decided: the reference's first five; min_stat between the third and fourth statistic
    stops after three; k > n; n = 1; an edge to the fixed vertex; a candidate whose Omega is indefinite is INFO_NOT_PD and
    never flagged; the size query through the C ABI leaves the outputs alone."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_manhattan(n_poses=400, side=20)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    ids = [int(i) for i in hg.vertices()[0]]
    fid, d, n = ids[0], 3, 300
    H0 = _oracle_of(hg).information(fid)
    Sig0 = np.linalg.inv(H0)
    poses = _poses(hg)
    far = _far_pairs(hg, n, seed=78)
    far[5] = (fid, ids[len(ids) // 2])
    rel = np.array([rr.between(d, poses[int(a)], poses[int(b)]) for a, b in far])
    T0 = sr.terms(d, poses, _at(ids, fid), far, rel, np.tile(rr.upper(np.eye(d)), (n, 1)))
    meas, info = [], []
    for i, t in enumerate(T0):
        ix, J = sr._support(t, d)
        s = BASE / (np.trace(J @ Sig0[np.ix_(ix, ix)] @ J.T) / d)
        off = np.array([np.sqrt(TARGET[0] * TARGET[1] ** min(i, TARGET[2]) / s), 0.0, 0.0])
        meas.append(rr.compose(d, rel[i], off))
        info.append(rr.upper(s * np.eye(d)))
    meas, info = np.array(meas), np.array(info)
    info[7] = rr.upper(info[7][0] * np.diag([1.0, -1.0, 1.0]))
    T = sr.terms(d, poses, _at(ids, fid), far, meas, info)
    ok = [t["ok"] for t in T]
    assert not ok[7] and sum(ok) == n - 1
    H1 = H0 + sum(t["A"].T @ t["Om"] @ t["A"] for t in T)
    Sig1 = np.linalg.inv(H1)
    geom = max(1.0, float(np.abs(g["poses"][:, :2]).max()), float(np.abs(meas[:, :2]).max()))
    single = _single_bounds(d, T, Sig1)
    single[7] = np.inf
    ref = orf.greedy_sigma(Sig1, T, ok, 5)
    bounds = _bounds(d, ref, T, single, geom)[0]
    assert _lead(ref, bounds) >= 1.0
    idx = _add_list(hg, far, meas, info)
    got = hg.detectOutliers(idx, 5, fixed_id=fid)
    _check_against(d, ref, T, single, geom, got, "manhattan 300")
    assert got["status"][7] == abi.OUTLIER_INFO_NOT_PD and np.isnan(got["final_stat"][7]) and np.isnan(got["final_margin"][7]) and np.isnan(got["redundancy"][7])
    mid = 0.5 * (ref["stat"][2] + ref["stat"][3])
    assert min(ref["stat"][2] - mid, mid - ref["stat"][3]) >= 10 * max(bounds[2][int(ref["flagged"][2])], bounds[3][int(ref["flagged"][3])])
    got3 = hg.detectOutliers(idx, 5, min_stat=mid, fixed_id=fid)
    assert got3["flagged"].tolist() == ref["flagged"][:3].tolist() and hg.last_covariance_stats["rounds"] == 3
    assert (got3["status"] == abi.OUTLIER_FLAGGED).sum() == 3
    _check_against(d, orf.greedy_sigma(Sig1, T, ok, 5, min_stat=mid), T, single, geom, got3, "manhattan 300, min_stat")
    # k > n: every usable candidate goes, then nothing is left
    few = idx[[5, 6, 7, 8, 9]]
    gotn = hg.detectOutliers(few, 9, fixed_id=fid)
    assert len(gotn["flagged"]) == 4 and sorted(gotn["flagged"].tolist()) == [0, 1, 3, 4] and np.array_equal(gotn["status"], [3, 3, 1, 3, 3])
    assert np.all(np.isnan(gotn["final_stat"]))
    # n = 1, and the edge to the fixed vertex alone
    first = int(ref["flagged"][0])
    got1 = hg.detectOutliers(idx[first:first + 1], 1, fixed_id=fid)
    assert got1["flagged"].tolist() == [0] and abs(got1["stat"][0] - ref["stat"][0]) <= bounds[0][first]
    gotf = hg.detectOutliers(idx[5:6], 1, fixed_id=fid)
    assert gotf["flagged"].tolist() == [0] and abs(gotf["stat"][0] - ref["rounds"][0][5][0]) <= bounds[0][5]
    # the size query: cap < min(k, n) and NULL outputs return min(k, n) and write nothing
    sel, cs = np.full(5, 77, np.int32), np.full(5, 7.0)
    ix = np.ascontiguousarray(idx)
    r = hg.L.spg_graph_detect_outliers(hg.h, fid, ix.ctypes.data_as(_i32p), n, 5, 0.0, 0.0, sel.ctypes.data_as(_i32p), cs.ctypes.data_as(_f64p), 4,
                                       None, None, None, None, None)
    assert r == 5 and np.all(sel == 77) and np.all(cs == 7.0)
    assert hg.L.spg_graph_detect_outliers(hg.h, fid, ix.ctypes.data_as(_i32p), n, 500, 0.0, 0.0, None, None, 0, None, None, None, None, None) == n
    # the tail beyond the return value is -1 / NaN
    sel, cs = np.full(5, 77, np.int32), np.full(5, 7.0)
    r = hg.L.spg_graph_detect_outliers(hg.h, fid, ix.ctypes.data_as(_i32p), n, 5, float(mid), 0.0, sel.ctypes.data_as(_i32p), cs.ctypes.data_as(_f64p), 5,
                                       None, None, None, None, None)
    assert r == 3 and sel[3:].tolist() == [-1, -1] and np.all(np.isnan(cs[3:])) and sel[:3].tolist() == ref["flagged"][:3].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_detection_leaves_the_graph_and_the_other_calls_untouched(d, hip_ctx):
    """detectOutliers does not modify the graph: the text of spg_graph_write_g2o_mem, the edges, the estimates and the outputs of pruneCandidates,
    selectCandidates and scoreCandidates are bit-identical before and after it."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    from tests.test_relative_covariance import _gate_candidates, _gate_graph
    g = _gate_graph(d)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    fid = int(g["ids"][0])
    ij, meas, info, _ = _gate_candidates(d, g)
    ij, meas, info = ij[:40], meas[:40], info[:40]
    cand = np.arange(0, hg.numEdges(), 7, dtype=np.int32)

    def calls():
        out = dict(hg.scoreCandidates(ij, meas, info, fixed_id=fid))
        out.update({"sel_" + k: v for k, v in hg.selectCandidates(ij, meas, info, 4, fixed_id=fid).items()})
        out.update({"prn_" + k: v for k, v in hg.pruneCandidates(cand, 5, fixed_id=fid).items()})
        return out
    before, e0, v0, txt0 = calls(), hg.edges(), hg.vertices(), hg.writeString()
    got = hg.detectOutliers(cand, 5, fixed_id=fid)
    assert len(got["flagged"]) == 5 and np.all(got["stat"] > 0)
    after, e1, v1, txt1 = calls(), hg.edges(), hg.vertices(), hg.writeString()
    assert txt0 == txt1
    for k in e0:
        assert np.array_equal(e0[k], e1[k]), k
    assert np.array_equal(v0[0], v1[0]) and np.array_equal(v0[1], v1[1])
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k


@pytest.mark.gpu
def test_cpp_facade_detection_matches_python(tmp_path, hip_ctx):
    """tests/cpp/outlier_demo.cpp flags 6 of every third edge of a small sphere through the facade and removes them; the
    indices, statistics, redundancies and statuses equal the Python binding's bit for bit."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_sphere(n_poses=200, ring=20)
    path = str(tmp_path / "s200.g2o")
    g2o_io.write_g2o(path, g)
    out = subprocess.run([_build_demo(tmp_path), path, "6", "0", str(tmp_path / "cpp.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and "outliers ok" in out.stdout, out.stdout + out.stderr
    lines = open(str(tmp_path / "cpp.txt")).read().split("\n")
    seq = np.array([[float(x) for x in ln.split()] for ln in lines if ln and not ln.startswith("r")]).reshape(-1, 2)
    per = np.array([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("r")]).reshape(-1, 3)
    hg = GraphWrapperHIP.load(path, ctx=hip_ctx)
    got = hg.detectOutliers(np.arange(0, hg.numEdges(), 3, dtype=np.int32), 6)
    assert len(seq) == 6 and np.array_equal(seq[:, 0].astype(np.int32), got["flagged"]) and np.array_equal(seq[:, 1], got["stat"])
    assert np.array_equal(per[:, 1], got["redundancy"], equal_nan=True) and np.array_equal(per[:, 2].astype(np.int32), got["status"])
