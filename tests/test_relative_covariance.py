"""Relative-pose covariances and loop-closure candidate scores (spg_graph_relative_covariances /
spg_graph_score_candidates, csrc/spg_sparse.inc: cov_solve_device, sp_relative_kernel) against the plain numpy formulas of
tests/relative_ref.py.
CPU: relative_ref against the multiprecision fixture, the log det identity of the gain in numpy alone, the argument and
capacity contract on an injected backend, the C++ demo compiles.
GPU: P = J Sigma_ab J^T and the relative pose against the dense inverse on small graphs (before and after marginalisation,
both gauges), the scores with their bounds, the gain against 1/2 delta log det of information() before and after addEdge,
the Mahalanobis gate on optimised graphs, the C++ façade.

Bounds (the issue's, not measured): with beta = ||J||inf^2 1e-9 max|Sigma| + 1e-11 max|P_ref| the bound on a pair's P (the
project's bound on a pair block, tests/test_pair_covariances.py, propagated through J, plus the cap of the device
geometry) and delta = D beta: |gain - ref| <= 1/2 D ||Omega||2 delta, |d2 - ref| <= chi2_ref ||Omega||2 delta (both from
M = I + L^T P L >= I), |chi2 - ref| <= 1e-11 max(1, chi2_ref).
Measured on an MI355X, worst error over its bound: P 1.5e-4 (manhattan_glc_tree; 3.6e-7 to 3.2e-6 on the other cases), rel
2.2e-5, gain 5.9e-9, d2 5.3e-10, chi2 1.2e-2; the gain against information() before and after addEdge 2.4e-10 of what is
allowed.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sparsifyposegraph_amd import abi, g2o_io
from sparsifyposegraph_amd.lib import SpgError
from tests import oracle_lib, util
from tests import relative_ref as rr
from tests.test_covariance_blocks import SMALL, _dense_blocks, _edge_pairs, _non_adjacent_pair, _oracle_of, _small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")
_f64p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
EINVAL, ESTATE = -1, -7
CHI2_99 = {3: 11.3449, 6: 16.8119}


# ------------------------------------------------------------------------------------------------------- CPU
def test_relative_ref_matches_the_multiprecision_reference():
    """relative_ref's error, Jacobians and relative pose over the case table of tests/golden/geometry_cases.npz (the
    float64-rounded outputs of tests/geom_ref.py), on the scales and within the bounds test_device_geometry.py holds the
    host restatement of the geometry to; with mpmath present, three cases per dimension against geom_ref itself."""
    from tests.test_device_geometry import ORACLE, SIGN_EXCLUDED, _cases, _miss
    worst = {"err": 0.0, "J": 0.0, "between": 0.0}
    for d in (6, 3):
        for name, c in _cases(d):
            if name in SIGN_EXCLUDED:
                continue
            e, Ji, Jj = rr.edge(d, c["xi"], c["xj"], c["z"])
            worst["err"] = max(worst["err"], _miss("err", e, c["ref_err"]))
            worst["J"] = max(worst["J"], _miss("J", Ji, c["ref_Ji"]), _miss("J", Jj, c["ref_Jj"]))
            worst["between"] = max(worst["between"], _miss("between", rr.between(d, c["xi"], c["xj"]), c["ref_between"]))
    print("relative_ref against the multiprecision reference: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= ORACLE[k], (k, v)
    try:
        from tests import geom_ref
    except ImportError:
        return
    for d in (6, 3):
        for name, c in _cases(d)[:3]:
            e, Ji, Jj = geom_ref.edge_terms(d, geom_ref.pose(d, c["xi"]), geom_ref.pose(d, c["xj"]), geom_ref.pose(d, c["z"]))
            got = rr.edge(d, c["xi"], c["xj"], c["z"])
            assert _miss("err", got[0], geom_ref.to_float(e)) <= ORACLE["err"]
            assert max(_miss("J", got[1], geom_ref.to_float(Ji)), _miss("J", got[2], geom_ref.to_float(Jj))) <= ORACLE["J"]


@pytest.mark.parametrize("d", [3, 6])
def test_gain_is_half_the_log_det_increase_in_numpy(d):
    """On a random SPD H over three poses: adding J^T Omega J of a binary edge between two of them raises ln det H by
    2 gain, gain = 1/2 ln det(I + Omega J Sigma_ab J^T) (matrix determinant lemma), and d2 <= chi2."""
    rng = np.random.default_rng(d)
    n = 3 * d
    A = rng.normal(size=(n, n))
    H = A @ A.T + n * np.eye(n)
    xs = [rng.normal(size=3) for _ in range(3)] if d == 3 else [np.concatenate([rng.normal(size=3), q / np.linalg.norm(q)])
                                                                 for q in rng.normal(size=(3, 4))]
    B = rng.normal(size=(d, d))
    Om = B @ B.T + np.eye(d)
    z = rr.compose(d, rr.between(d, xs[0], xs[2]), rr.from_mqt(0.05 * rng.normal(size=6)) if d == 6 else 0.05 * rng.normal(size=3))
    Sig = np.linalg.inv(H)
    idx = np.r_[0:d, 2 * d:3 * d]
    e, J, P = rr.error_covariance(d, xs[0], xs[2], z, Sig[np.ix_(idx, idx)])
    d2, gain, chi2 = rr.scores(e, P, Om)
    Jf = np.zeros((d, n))
    Jf[:, idx] = J
    want = 0.5 * (np.linalg.slogdet(H + Jf.T @ Om @ Jf)[1] - np.linalg.slogdet(H)[1])
    assert abs(gain - want) <= 1e-12 * max(1.0, abs(want))
    assert 0 < d2 <= chi2 * (1 + 1e-12)
    # the posterior chi2 of the new edge alone: e^T (P + Omega^-1)^-1 e through the updated information
    S2 = np.linalg.inv(H + Jf.T @ Om @ Jf)
    assert d2 == pytest.approx(e @ (Om - Om @ Jf @ S2 @ Jf.T @ Om) @ e, rel=1e-9)


def test_relative_calls_check_arguments_before_the_backend():
    """On an injected (CPU) context: the size queries answer; an unknown id, a == b, an unknown fixed vertex, a non-finite
    measurement and an active stepwise marginalisation are SPG_EINVAL with the pair named; a call that would compute is
    SPG_ESTATE (no CPU fallback)."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    sub = _small()
    ictx = oracle_lib.injected_context()
    a = GraphWrapperHIP.from_dict(sub, ctx=ictx)
    L, D = a.L, 3
    ids = np.ascontiguousarray(sub["ids"][:5], np.int32)
    na = np.array(_non_adjacent_pair(sub), np.int32)
    e0 = [int(x) for x in sub["edge_ij"][0]]
    pairs = np.array([e0, list(na), list(na), [na[1], na[0]]], np.int32)
    n = len(pairs)
    rec = np.ascontiguousarray(np.tile(sub["edge_data"][0], (n, 1)))
    buf, rel = np.zeros(4096), np.zeros(4096)
    out = [np.zeros(n) for _ in range(3)]
    status = np.zeros(n, np.int32)
    f = lambda x: x.ctypes.data_as(_f64p)  # noqa: E731
    i = lambda x: x.ctypes.data_as(_i32p)  # noqa: E731
    score = lambda ij, r, k, cap, fid=-1: L.spg_graph_score_candidates(a.h, fid, i(ij), f(r), k, f(out[0]), f(out[1]), f(out[2]), i(status),  # noqa: E731
                                                                       cap, None)
    # size queries
    assert L.spg_graph_relative_covariances(a.h, -1, i(pairs), n, None, None, 0, None) == n * D * D
    assert L.spg_graph_relative_covariances(a.h, -1, i(pairs), n, f(rel), f(buf), n * D * D - 1, None) == n * D * D
    assert L.spg_graph_relative_covariances(a.h, -1, i(pairs), 0, None, None, 0, None) == 0
    assert score(pairs, rec, n, 0) == n and score(pairs, rec, n, n - 1) == n
    # no HIP backend
    st = abi.CovSolveStats()
    assert L.spg_graph_relative_covariances(a.h, -1, i(pairs), n, f(rel), f(buf), buf.size, C.byref(st)) == ESTATE
    assert L.spg_graph_relative_covariances(a.h, -1, i(pairs), n, None, f(buf), buf.size, None) == ESTATE
    assert score(pairs, rec, n, n) == ESTATE
    # invalid arguments, answered before the backend
    unknown = np.array([int(ids[0]), 999999], np.int32)
    same = np.array([e0[0], e0[0]], np.int32)
    for bad, word in ((unknown, "999999"), (same, "same")):
        assert L.spg_graph_relative_covariances(a.h, -1, i(bad), 1, None, None, 0, None) == EINVAL
        assert word in L.spg_last_error(ictx.h).decode()
        assert score(bad, rec, 1, 0) == EINVAL
        assert word in L.spg_last_error(ictx.h).decode()
    assert L.spg_graph_relative_covariances(a.h, 999999, i(pairs), n, None, None, 0, None) == EINVAL
    assert "fixed vertex" in L.spg_last_error(ictx.h).decode()
    assert score(pairs, rec, n, 0, fid=999999) == EINVAL
    for bad_value in (np.nan, np.inf):
        r2 = rec.copy()
        r2[2, 1] = bad_value
        assert score(pairs, r2, n, 0) == EINVAL
        msg = L.spg_last_error(ictx.h).decode()
        assert "pair 2" in msg and f"({na[0]}, {na[1]})" in msg and "finite" in msg
    r2 = rec.copy()
    r2[1, D:] = np.nan          # a non-finite information is a status of the candidate, not an argument error
    assert score(pairs, r2, n, 0) == n
    assert L.spg_graph_score_candidates(a.h, -1, i(pairs), None, n, None, None, None, None, 0, None) == EINVAL
    # an active stepwise marginalisation
    g, which, opts, *_ = util.load_golden("intel_nfr_tree_sp3")
    sub2, w = util.prefix_graph(g, which, 30)
    b = GraphWrapperHIP.from_dict(sub2, ctx=ictx)
    b.begin(w, opts, 0, 1)
    assert L.spg_graph_relative_covariances(b.h, -1, i(pairs), n, None, None, 0, None) == EINVAL
    assert "active" in L.spg_last_error(ictx.h).decode()
    assert L.spg_graph_score_candidates(b.h, -1, i(pairs), f(rec), n, None, None, None, None, 0, None) == EINVAL
    # the Python layer raises for each
    with pytest.raises(SpgError, match="HIP backend"):
        a.relativeCovariances(pairs)
    with pytest.raises(SpgError, match="HIP backend"):
        a.scoreCandidates(pairs, rec[:, :D], rec[:, D:])
    with pytest.raises(SpgError, match="not in the graph"):
        a.relativeCovariances([unknown])
    with pytest.raises(SpgError, match="same"):
        a.scoreCandidates([same], rec[:1, :D], rec[:1, D:])
    with pytest.raises(SpgError, match="fixed vertex"):
        a.relativeCovariances(pairs, fixed_id=999999)
    with pytest.raises(ValueError):
        a.scoreCandidates(pairs, rec[:, :D], rec[:, D:-1])


def _build_demo(tmp_path):
    exe = str(tmp_path / "candidate_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "candidate_demo.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_candidate_demo_compiles(tmp_path):
    out = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr


# ---- the gate's candidates
GATE_SEED = {3: 5, 6: 6}


def _gate_graph(d):
    return g2o_io.synth_manhattan(n_poses=400, side=20) if d == 3 else g2o_io.synth_sphere(n_poses=400, ring=20)


def _rot_angle_deg(d, za, zb):
    """angle of the rotation za^-1 zb"""
    if d == 3:
        return abs(np.degrees(rr.normalize_theta(zb[2] - za[2])))
    w = abs(float(np.dot(za[3:], zb[3:])))
    return np.degrees(2 * np.arccos(min(1.0, w)))


def _gate_candidates(d, g):
    """50 inliers (the true relative pose of a random pair composed with noise drawn from Omega = the generator's information)
    and 50 outliers (the true relative pose of a different pair whose relative translation differs by at least 10 and whose
    rotation differs by less than 90 degrees, well under the 120 at which an SE3 error nears the quaternion sign change).
    The generator's poses are the truth. Returns (ij[100, 2], meas, info_upper, inlier[100])."""
    rng = np.random.default_rng(GATE_SEED[d])
    truth, ids = g["poses"], g["ids"]
    info_upper = g["edge_data"][0, abi.pose_stride(d):]
    sig = 1.0 / np.sqrt(np.diag(rr.omega(d, info_upper)))
    ij, meas = [], []

    def pair():
        a, b = rng.choice(len(ids), size=2, replace=False)
        return int(a), int(b)
    for _ in range(50):
        a, b = pair()
        nz = rng.normal(size=d) * sig
        ij.append((ids[a], ids[b]))
        meas.append(rr.compose(d, rr.between(d, truth[a], truth[b]), rr.from_mqt(nz) if d == 6 else nz))
    while len(ij) < 100:
        a, b = pair()
        c, e = pair()
        za, zc = rr.between(d, truth[a], truth[b]), rr.between(d, truth[c], truth[e])
        tl = 2 if d == 3 else 3
        if np.linalg.norm(za[:tl] - zc[:tl]) < 10.0 or _rot_angle_deg(d, za, zc) >= 90.0:
            continue
        ij.append((ids[a], ids[b]))
        meas.append(zc)
    return np.array(ij, np.int32), np.array(meas), np.tile(info_upper, (100, 1)), np.arange(100) < 50


def _ref_scores(d, poses_of, blk, ij, meas, info_upper):
    """relative_ref over a candidate list. poses_of: id -> pose, blk: (a, b) -> Sigma block. Returns dict of arrays plus
    beta (the bound on P), ||Omega||2 and P."""
    out = {k: np.zeros(len(ij)) for k in ("d2", "gain", "chi2", "beta", "om2")}
    out["P"] = np.zeros((len(ij), d, d))
    for k, (a, b) in enumerate(ij):
        a, b = int(a), int(b)
        S = np.block([[blk(a, a), blk(a, b)], [blk(b, a), blk(b, b)]])
        e, J, P = rr.error_covariance(d, poses_of[a], poses_of[b], meas[k], S)
        Om = rr.omega(d, info_upper[k])
        out["P"][k] = P
        out["beta"][k] = np.abs(J).sum(axis=1).max() ** 2 * 1e-9 * blk.scale + 1e-11 * np.abs(P).max()
        if np.all(np.isfinite(Om)) and np.linalg.eigvalsh(Om).min() > 0:
            out["d2"][k], out["gain"][k], out["chi2"][k] = rr.scores(e, P, Om)
            out["om2"][k] = np.linalg.norm(Om, 2)
        else:
            out["d2"][k] = out["gain"][k] = out["chi2"][k] = out["om2"][k] = np.nan
    return out


def _blocks_of(og, ids, fid, d):
    Sig = np.linalg.inv(og.information(fid))
    blk = _dense_blocks(Sig, ids, fid, d)
    blk.scale = float(np.abs(Sig).max())
    return blk


# ------------------------------------------------------------------------------------------------------- GPU
def _far_pairs(hg, k, seed):
    """k random vertex pairs without a common edge."""
    ids = [int(i) for i in hg.vertices()[0]]
    adj = {tuple(p) for p in _edge_pairs(hg).tolist()}
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < k:
        a, b = (int(x) for x in rng.choice(ids, size=2, replace=False))
        if (min(a, b), max(a, b)) not in adj:
            out.append((a, b))
    return np.array(out, np.int32)


def _poses_of(hg):
    ids, poses = hg.vertices()
    return {int(i): np.array(p) for i, p in zip(ids, poses)}


def _small_graphs(case, n, hip_ctx):
    """(graph, oracle twin) of a SMALL case before and after its marginalisation, and the kept ids"""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, which, opts, *_ = util.load_golden(case)
    sub, w = util.prefix_graph(g, which, n)
    base = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx)
    sp = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx, useGLC=opts.algorithm == abi.ALG_GLC)
    st = sp.marginalizeNoOptimize(w, opts)
    assert st["n_bad_status"] == 0 and st["n_removed"] == len(w)
    kept = [int(i) for i in sp.vertices()[0]]
    return sub, ((base, oracle_lib.OracleGraph.from_dict(sub)), (sp, _oracle_of(sp))), kept


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", SMALL)
def test_relative_covariances_equal_the_dense_inverse_on_small_graphs(case, n, hip_ctx):
    """P and rel of 40 far pairs, every edge pair, one vertex against all others, pairs with the fixed vertex as a and as b
    and one pair listed three times, against relative_ref on inv(oracle information), within beta; P bit-for-bit
    symmetric, repeats bit-identical, one solved column for the star."""
    sub, graphs, kept = _small_graphs(case, n, hip_ctx)
    D = sub["pose_dim"]
    worst, worst_rel = 0.0, 0.0
    for hg, og in graphs:
        ids = [int(i) for i in hg.vertices()[0]]
        poses = _poses_of(hg)
        for fid in (ids[0], kept[len(kept) // 2]):
            blk = _blocks_of(og, ids, fid, D)
            far = _far_pairs(hg, 40, seed=fid)
            v0 = ids[len(ids) // 3]
            star = np.array([(v0, v) for v in ids if v != v0], np.int32)
            other = next(v for v in ids if v != fid)
            with_fixed = np.array([(fid, other), (other, fid), (fid, ids[-1] if ids[-1] != fid else ids[-2])], np.int32)
            thrice = np.array([far[7]] * 3, np.int32)
            pairs = np.concatenate([far, _edge_pairs(hg), star, with_fixed, thrice])
            rel, P = hg.relativeCovariances(pairs, fixed_id=fid)
            assert np.array_equal(P, P.transpose(0, 2, 1))
            assert np.array_equal(P[-3], P[-2]) and np.array_equal(P[-3], P[-1]) and np.array_equal(P[-3], P[7])
            assert np.array_equal(rel[-3], rel[-1]) and np.array_equal(rel[-3], rel[7])
            for k, (a, b) in enumerate(pairs):
                a, b = int(a), int(b)
                S = np.block([[blk(a, a), blk(a, b)], [blk(b, a), blk(b, b)]])
                rel_ref, J, P_ref = rr.relative_covariance(D, poses[a], poses[b], S)
                beta = np.abs(J).sum(axis=1).max() ** 2 * 1e-9 * blk.scale + 1e-11 * np.abs(P_ref).max()
                err = np.abs(P[k] - P_ref).max()
                worst = max(worst, err / beta)
                assert err <= beta, (case, hg is graphs[1][0], fid, a, b, err / beta)
                erel = np.abs(rel[k] - rel_ref).max() / (1e-11 * np.linalg.norm(rel_ref))
                worst_rel = max(worst_rel, erel)
                assert erel <= 1.0, (case, fid, a, b, erel)
            # the star alone: one solved column; the relative poses do not depend on the list they are asked in
            rel_s, _ = hg.relativeCovariances(star, fixed_id=fid)
            s = hg.last_covariance_stats
            assert s["columns"] == 1 and s["rhs_batches"] == 1 and s["device_seconds"] > s["solve_seconds"] > 0
            o = 40 + len(_edge_pairs(hg))
            assert np.array_equal(rel_s, rel[o:o + len(star)])
    print(f"{case}[{n}]: worst P error / beta {worst:.2e}, worst rel error / (1e-11 |rel|) {worst_rel:.2e}")


def _perturbed(d, rel, Om, s, rng):
    """rel composed with a perturbation of Mahalanobis length s under Om"""
    u = rng.normal(size=d)
    dlt = s * np.linalg.solve(np.linalg.cholesky(Om).T, u / np.linalg.norm(u))
    return rr.compose(d, rel, rr.from_mqt(dlt) if d == 6 else dlt)


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", SMALL)
def test_candidate_scores_equal_the_dense_formulas_on_small_graphs(case, n, hip_ctx):
    """d2, gain and chi2 of candidates between far pairs (Omega of a random existing edge, z = the current relative pose
    composed with 0 to 4 sigma) within the bounds of the header; a candidate whose Omega has a negative eigenvalue and one
    whose Omega is NaN report SPG_CAND_INFO_NOT_PD and NaN without touching the others; at z = the current relative pose the
    gain equals 1/2 ln det(I + Omega P) of relativeCovariances' P."""
    sub, graphs, kept = _small_graphs(case, n, hip_ctx)
    D, ps = sub["pose_dim"], abi.pose_stride(sub["pose_dim"])
    worst = {"gain": 0.0, "d2": 0.0, "chi2": 0.0}
    for hg, og in graphs:
        ids = [int(i) for i in hg.vertices()[0]]
        poses = _poses_of(hg)
        for fid in (ids[0], kept[len(kept) // 2]):
            rng = np.random.default_rng(fid + 1)
            blk = _blocks_of(og, ids, fid, D)
            far = _far_pairs(hg, 40, seed=fid)
            far[3] = (fid, next(v for v in reversed(ids) if v != fid))
            rel, P0 = hg.relativeCovariances(far, fixed_id=fid)
            info = sub["edge_data"][rng.integers(len(sub["edge_data"]), size=len(far)), ps:].copy()
            meas = np.array([_perturbed(D, rel[k], rr.omega(D, info[k]), 4.0 * rng.random(), rng) for k in range(len(far))])
            # 30 .. 39: measured at the current relative pose exactly as the device reported it
            meas[30:] = rel[30:]
            bad_neg, bad_nan = 11, 23
            all_good = hg.scoreCandidates(far, meas, info, fixed_id=fid)
            Om = rr.omega(D, info[bad_neg])
            w, V = np.linalg.eigh(Om)
            w[0] = -0.5 * w[1]
            info[bad_neg] = rr.upper(V @ np.diag(w) @ V.T)
            info[bad_nan] = np.nan
            got = hg.scoreCandidates(far, meas, info, fixed_id=fid)
            ref = _ref_scores(D, poses, blk, far, meas, info)
            bad = np.zeros(len(far), bool)
            bad[[bad_neg, bad_nan]] = True
            assert np.array_equal(got["status"], np.where(bad, abi.CAND_INFO_NOT_PD, abi.CAND_SCORED))
            for k in ("d2", "gain", "chi2"):
                assert np.all(np.isnan(got[k][bad])) and np.all(np.isfinite(got[k][~bad]))
            # the others are unaffected: the same bits as in the same list with a usable Omega in those two places
            assert np.array_equal(all_good["status"], np.zeros(len(far), np.int32))
            for k in ("d2", "gain", "chi2"):
                assert np.array_equal(all_good[k][~bad], got[k][~bad]) and np.all(np.isfinite(all_good[k]))
            delta = D * ref["beta"]
            for k in np.flatnonzero(~bad):
                bg = 0.5 * D * ref["om2"][k] * delta[k]
                worst["gain"] = max(worst["gain"], abs(got["gain"][k] - ref["gain"][k]) / bg)
                assert abs(got["gain"][k] - ref["gain"][k]) <= bg, (case, fid, k)
                bc = 1e-11 * max(1.0, ref["chi2"][k])
                worst["chi2"] = max(worst["chi2"], abs(got["chi2"][k] - ref["chi2"][k]) / bc)
                assert abs(got["chi2"][k] - ref["chi2"][k]) <= bc, (case, fid, k)
                if k < 30:
                    bd = ref["chi2"][k] * ref["om2"][k] * delta[k]
                    worst["d2"] = max(worst["d2"], abs(got["d2"][k] - ref["d2"][k]) / bd)
                    assert abs(got["d2"][k] - ref["d2"][k]) <= bd, (case, fid, k, got["d2"][k], ref["d2"][k], bd)
                else:
                    # e is zero up to the rounding of one ulp of the pose: so are chi2 and d2, and d2 <= chi2
                    assert 0.0 <= got["d2"][k] <= got["chi2"][k] * (1 + 1e-12) and got["chi2"][k] <= 1e-11
                    via_P = 0.5 * np.linalg.slogdet(np.eye(D) + rr.omega(D, info[k]) @ P0[k])[1]
                    assert abs(got["gain"][k] - via_P) <= bg, (case, fid, k)
    print(f"{case}[{n}]: worst error / bound: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_zero_error_gives_zero_distance_exactly(d, hip_ctx):
    """Three poses without rotation at integer positions: a candidate measured at the relative pose has e = 0 in every bit,
    and then chi2 == 0 and d2 == 0 exactly while the gain is positive."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    ps = abi.pose_stride(d)
    poses = np.zeros((3, ps))
    poses[:, :2] = [[0, 0], [3, 1], [5, -2]]
    if d == 6:
        poses[:, 6] = 1.0
    info = rr.upper(np.diag(np.arange(1.0, d + 1)) + 0.25)
    edges = np.array([[0, 1], [1, 2]], np.int32)
    data = np.array([np.concatenate([rr.between(d, poses[a], poses[b]), info]) for a, b in edges])
    hg = GraphWrapperHIP.from_dict({"pose_dim": d, "ids": np.arange(3, dtype=np.int32), "poses": poses, "edge_ij": edges, "edge_data": data}, ctx=hip_ctx)
    ij = np.array([[0, 2], [2, 0], [0, 1]], np.int32)
    rel, P = hg.relativeCovariances(ij)
    assert np.array_equal(rel, np.array([rr.between(d, poses[a], poses[b]) for a, b in ij]))
    got = hg.scoreCandidates(ij, rel, np.tile(info, (3, 1)))
    assert np.array_equal(got["status"], np.zeros(3, np.int32))
    assert np.array_equal(got["chi2"], np.zeros(3)) and np.array_equal(got["d2"], np.zeros(3))
    assert np.all(got["gain"] > 0)
    for k in range(3):
        assert got["gain"][k] == pytest.approx(0.5 * np.linalg.slogdet(np.eye(d) + rr.omega(d, info) @ P[k])[1], rel=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_gain_equals_half_the_log_det_increase_of_information(d, hip_ctx):
    """Through the product's own assembly: for 5 candidates on a small graph, 1/2 (ln det information() after addEdge of
    the candidate on a copy - ln det information() before) against the device gain. Allowed: the gain's bound plus the
    deviation of relative_ref's own gain from the same quantity (measured here; the reference is not code under test)."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    if d == 3:
        sub = _small(30)
    else:
        g, which, *_ = util.load_golden("sphere_nfr_tree")
        sub, _ = util.prefix_graph(g, which, 40)
    ps = abi.pose_stride(d)
    hg = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx)
    ids = [int(i) for i in hg.vertices()[0]]
    fid = ids[0]
    H = hg.information(fid)
    ld0 = np.linalg.slogdet(H)[1]
    Sig = np.linalg.inv(H)
    blk = _dense_blocks(Sig, ids, fid, d)
    blk.scale = float(np.abs(Sig).max())
    rng = np.random.default_rng(d)
    ij = _far_pairs(hg, 5, seed=d)
    ij[0] = (fid, ij[0][1] if ij[0][1] != fid else ids[-1])
    rel, _ = hg.relativeCovariances(ij, fixed_id=fid)
    info = sub["edge_data"][rng.integers(len(sub["edge_data"]), size=5), ps:]
    meas = np.array([_perturbed(d, rel[k], rr.omega(d, info[k]), 4.0 * rng.random(), rng) for k in range(5)])
    got = hg.scoreCandidates(ij, meas, info, fixed_id=fid)
    ref = _ref_scores(d, _poses_of(hg), blk, ij, meas, info)
    worst = 0.0
    for k in range(5):
        h2 = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx)
        h2.addEdge(int(ij[k][0]), int(ij[k][1]), meas[k], info[k])
        want = 0.5 * (np.linalg.slogdet(h2.information(fid))[1] - ld0)
        allowed = 0.5 * d * ref["om2"][k] * d * ref["beta"][k] + abs(ref["gain"][k] - want)
        worst = max(worst, abs(got["gain"][k] - want) / allowed)
        assert want > 0 and abs(got["gain"][k] - want) <= allowed, (k, got["gain"][k], want, allowed)
    assert hg.numEdges() == len(sub["edge_ij"])      # scoring does not modify the graph
    print(f"D={d}: gain against 1/2 delta log det of information(): worst deviation / allowed {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_mahalanobis_gate_separates_inliers_from_outliers(d, hip_ctx):
    """A synth_manhattan / synth_sphere graph of 400 poses after optimize(50): of 50 inlier candidates (the true relative
    pose plus noise drawn from Omega) at least 45 pass d2 < the 99 % chi^2 quantile, every one of 50 outliers (the true
    relative pose of a different, distant pair) fails it, and the device agrees with relative_ref on every candidate.
    The seeds were chosen with relative_ref alone on the oracle's optimised graph (no device): SE2 49 of 50 inliers accepted,
    smallest outlier d2 50.7, no d2 closer to the quantile than 1.5e-2 (relative); SE3 49 of 50, 22.9 and 7.8e-2; every SE3
    outlier's error rotation below 120 degrees."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = _gate_graph(d)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    fid = int(g["ids"][0])
    hg.optimize(50, fixed_id=fid)
    ids = [int(i) for i in hg.vertices()[0]]
    ij, meas, info, inlier = _gate_candidates(d, g)
    got = hg.scoreCandidates(ij, meas, info, fixed_id=fid)
    ref = _ref_scores(d, _poses_of(hg), _blocks_of(_oracle_of(hg), ids, fid, d), ij, meas, info)
    q = CHI2_99[d]
    print(f"D={d}: inliers accepted {int((got['d2'][inlier] < q).sum())}/50, smallest outlier d2 {got['d2'][~inlier].min():.1f}, "
          f"worst |d2 - ref| / ref {np.abs(got['d2'] / ref['d2'] - 1).max():.1e}")
    assert np.array_equal(got["status"], np.zeros(100, np.int32))
    assert np.array_equal(got["d2"] < q, ref["d2"] < q)
    assert np.all(got["d2"][~inlier] >= q)
    assert (got["d2"][inlier] < q).sum() >= 45


@pytest.mark.gpu
def test_cpp_facade_candidates_match_python(tmp_path, hip_ctx):
    """tests/cpp/candidate_demo.cpp calls the façade's relativeCovariances / scoreCandidates on a small sphere and prints
    the results; they equal the Python binding's bit for bit."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_sphere(n_poses=200, ring=20)
    path = str(tmp_path / "s200.g2o")
    g2o_io.write_g2o(path, g)
    out = subprocess.run([_build_demo(tmp_path), path, str(tmp_path / "cpp.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.loadtxt(str(tmp_path / "cpp.txt"))
    hg = GraphWrapperHIP.load(path, ctx=hip_ctx)
    ids = [int(i) for i in hg.vertices()[0]]
    n = len(ids)
    pairs = np.array([(ids[0], ids[i]) for i in range(1, n)] + [(ids[i], ids[n - 1 - i]) for i in range(n // 2)], np.int32)
    rel, P = hg.relativeCovariances(pairs)
    e = hg.edges()
    k = next(k for k in range(len(e["kind"])) if ids[0] in e["vert_ids"][e["vert_off"][k]:e["vert_off"][k + 1]])
    info = e["data"][e["data_off"][k] + 7:e["data_off"][k + 1]]
    s = hg.scoreCandidates(pairs, np.roll(rel, -1, axis=0), np.tile(info, (len(pairs), 1)))
    ref = np.concatenate([np.concatenate([rel, P.reshape(len(pairs), -1)], axis=1).ravel(),
                          np.stack([s["d2"], s["gain"], s["chi2"], s["status"].astype(np.float64)], axis=1).ravel()])
    assert got.shape == ref.shape and np.array_equal(got, ref)
    assert "candidates ok" in out.stdout
