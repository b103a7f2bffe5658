"""Covariance of arbitrary pose pairs and pose sets from the sparse factor (spg_graph_pair_covariances /
spg_graph_joint_marginal_covariance, csrc/spg_sparse.inc: ColumnSolves, sp_panel_rows_kernel, sp_cov_assemble_kernel) —
iSAM's covariances().marginal(list) as GraphWrapperISAM::covariance asks for it (src/graph_wrapper_isam.cpp:259-262).
CPU: argument checking before the backend, and a numpy restatement of the path-pruned column solve on the plan's arrays.
GPU: numpy's inv(H) on small graphs (before and after marginalisation, both gauges) with the bit-for-bit invariants
against the selected inverse, the dense covariance() on sphere.g2o at full size, the exactness of GLC Dense /
CliqueyDense across graphs, the headline size (and the solves forced onto in-pattern blocks), the C++ façade."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from sparsifyposegraph_amd import abi, g2o_io
from sparsifyposegraph_amd.lib import SpgError, sparse_plan
from tests import oracle_lib, util
from tests.test_covariance_blocks import SMALL, _dense_blocks, _edge_pairs, _exact_case, _non_adjacent_pair, _oracle_of, _small
from tests.test_sparse_plan import lattice, multifrontal, random_spd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")
_f64p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
EINVAL, ESTATE, ECAPACITY = -1, -7, -4


# ------------------------------------------------------------------------------------------------------- CPU
def test_pair_and_set_calls_check_arguments_before_the_backend():
    """On an injected (CPU) context: the size queries answer (non-adjacent pairs included), unknown ids, a == b, duplicate
    set ids and an unknown fixed vertex are SPG_EINVAL, a set above 46 000 variables is SPG_ECAPACITY, and a call that
    would compute is SPG_ESTATE (no CPU fallback)."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    sub = _small()
    ictx = oracle_lib.injected_context()
    a = GraphWrapperHIP.from_dict(sub, ctx=ictx)
    L, D = a.L, 3
    ids = np.ascontiguousarray(sub["ids"][:5], np.int32)
    na = np.array(_non_adjacent_pair(sub), np.int32)
    e0 = [int(x) for x in sub["edge_ij"][0]]
    pairs = np.array([e0, list(na), [na[1], na[0]]], np.int32)
    buf = np.zeros(4096)
    f = lambda x: x.ctypes.data_as(_f64p)  # noqa: E731
    i = lambda x: x.ctypes.data_as(_i32p)  # noqa: E731
    # size queries
    assert L.spg_graph_pair_covariances(a.h, -1, i(na), 1, None, 0, None) == (2 * D) ** 2
    assert L.spg_graph_pair_covariances(a.h, -1, i(pairs), 3, None, 0, None) == 3 * (2 * D) ** 2
    assert L.spg_graph_pair_covariances(a.h, -1, i(pairs), 3, f(buf), 3 * (2 * D) ** 2 - 1, None) == 3 * (2 * D) ** 2
    assert L.spg_graph_joint_marginal_covariance(a.h, -1, i(ids), 5, None, 0, None) == (5 * D) ** 2
    assert L.spg_graph_joint_marginal_covariance(a.h, -1, i(ids), 0, None, 0, None) == 0
    # no HIP backend
    st = abi.CovSolveStats()
    assert L.spg_graph_pair_covariances(a.h, -1, i(pairs), 3, f(buf), buf.size, C.byref(st)) == ESTATE
    assert L.spg_graph_joint_marginal_covariance(a.h, -1, i(ids), 5, f(buf), buf.size, C.byref(st)) == ESTATE
    # invalid arguments, answered before the backend
    unknown = np.array([int(ids[0]), 999999], np.int32)
    assert L.spg_graph_pair_covariances(a.h, -1, i(unknown), 1, None, 0, None) == EINVAL
    assert "999999" in L.spg_last_error(ictx.h).decode()
    assert L.spg_graph_joint_marginal_covariance(a.h, -1, i(unknown), 2, None, 0, None) == EINVAL
    same = np.array([e0[0], e0[0]], np.int32)
    assert L.spg_graph_pair_covariances(a.h, -1, i(same), 1, None, 0, None) == EINVAL
    assert "same" in L.spg_last_error(ictx.h).decode()
    dup = np.array([ids[0], ids[1], ids[0]], np.int32)
    assert L.spg_graph_joint_marginal_covariance(a.h, -1, i(dup), 3, None, 0, None) == EINVAL
    assert "twice" in L.spg_last_error(ictx.h).decode()
    assert L.spg_graph_pair_covariances(a.h, 999999, i(pairs), 3, None, 0, None) == EINVAL
    assert L.spg_graph_joint_marginal_covariance(a.h, 999999, i(ids), 5, None, 0, None) == EINVAL
    big = np.arange(46000 // D + 1, dtype=np.int32)
    assert L.spg_graph_joint_marginal_covariance(a.h, -1, i(big), len(big), None, 0, None) == ECAPACITY
    # the existing edge-pair call keeps refusing the non-adjacent pair
    assert L.spg_graph_joint_covariances(a.h, -1, i(na), 1, None, 0, None) == EINVAL
    # the Python layer raises for each
    with pytest.raises(SpgError, match="HIP backend"):
        a.pairCovariances(pairs)
    with pytest.raises(SpgError, match="HIP backend"):
        a.jointMarginalCovariance(ids)
    with pytest.raises(SpgError, match="not in the graph"):
        a.pairCovariances([unknown])
    with pytest.raises(SpgError, match="same"):
        a.pairCovariances([same])
    with pytest.raises(SpgError, match="twice"):
        a.jointMarginalCovariance(dup)
    with pytest.raises(SpgError, match="fixed vertex"):
        a.jointMarginalCovariance(ids, fixed_id=999999)
    with pytest.raises(SpgError, match="46k"):
        a.jointMarginalCovariance(big)


def _plan_case(R, Cc, D, leaf, seed):
    """A lattice with random n-ary cliques (3 to 5 blocks), its plan over the graph's own order, a random SPD H on that
    pattern and the numpy multifrontal factor."""
    _, _, pairs = lattice(R, Cc, 3, seed=seed)
    n = R * Cc
    rng = np.random.default_rng(seed + D)
    allp = set(pairs)
    for _ in range(5):
        c = sorted(int(x) for x in rng.choice(n, size=int(rng.integers(3, 6)), replace=False))
        allp.update((a, b) for x, a in enumerate(c) for b in c[x + 1:])
    adj = [[] for _ in range(n)]
    for a, b in allp:
        adj[a].append(b)
        adj[b].append(a)
    ptr = np.zeros(n + 1, np.int32)
    ptr[1:] = np.cumsum([len(x) for x in adj])
    plan = sparse_plan(ptr, np.array([u for x in adj for u in sorted(x)], np.int32), D, leaf=leaf)
    H = random_spd(n, D, sorted(allp), seed=seed)
    fronts, _, NP, NB, iperm, _ = multifrontal(plan, H, D)
    return plan, H, fronts, NP, NB, iperm


def _root_path(plan, s):
    out = []
    while s >= 0:
        out.append(s)
        s = plan["parent"][s]
    return out


def _pruned_column(plan, fronts, NP, D, iperm, b, rows, skip_fw=None, skip_bw=None):
    """Sigma[rows, b] by the device's column solve: forward L y = E_b over b's root path only (children's update rows
    extend-added in child order), backward L^T x = y over the rows' root paths only (boundary values gathered from the
    parent's panel). skip_fw / skip_bw: a front left out of one sweep."""
    first, parent, rowptr, rel = plan["first"], plan["parent"], plan["rowptr"], plan["rel"]
    nsn = len(first) - 1
    sn_of = np.repeat(np.arange(nsn), np.diff(first))
    fw = set(_root_path(plan, sn_of[iperm[b]]))
    bw = set().union(*(_root_path(plan, sn_of[iperm[a]]) for a in rows))
    W = {s: np.zeros((fronts[s].shape[0], D)) for s in fw | bw}
    sb, qb = sn_of[iperm[b]], iperm[b]
    W[sb][D * (qb - first[sb]):D * (qb - first[sb]) + D] = np.eye(D)
    fw.discard(skip_fw)
    bw.discard(skip_bw)
    idx = lambda c: np.concatenate([np.arange(x, x + D) for x in rel[rowptr[c]:rowptr[c + 1]]])  # noqa: E731
    for s in sorted(fw):                 # children come before their parent
        for c in sorted(fw):
            if parent[c] == s:
                nr = D * (rowptr[c + 1] - rowptr[c])
                W[s][idx(c)] += W[c][NP[c]:NP[c] + nr]
        F, np_ = fronts[s], NP[s]
        W[s][:np_] = np.linalg.solve(np.tril(F[:np_, :np_]), W[s][:np_])
        W[s][np_:] -= F[np_:, :np_] @ W[s][:np_]
    for s in sorted(bw, reverse=True):
        F, np_ = fronts[s], NP[s]
        if parent[s] >= 0:
            nr = D * (rowptr[s + 1] - rowptr[s])
            W[s][np_:np_ + nr] = W[parent[s]][idx(s)]
        W[s][:np_] = np.linalg.solve(np.tril(F[:np_, :np_]).T, W[s][:np_] - F[np_:, :np_].T @ W[s][np_:])
    out = []
    for a in rows:
        s, q = sn_of[iperm[a]], iperm[a]
        out.append(W[s][D * (q - first[s]):D * (q - first[s]) + D])
    return np.array(out), fw | {skip_fw} - {None}, bw | {skip_bw} - {None}


@pytest.mark.parametrize("R,Cc,D,leaf,seed", [(9, 10, 3, 6, 1), (7, 8, 6, 5, 2), (12, 6, 3, 4, 3), (6, 9, 6, 1000, 4)])
def test_pruned_column_solve_restated_in_numpy(R, Cc, D, leaf, seed):
    """A forward sweep over the column's root path and a backward sweep over the requested rows' root paths reproduce
    those blocks of inv(H); leaving any single front out of either path changes the result (the paths are not larger
    than needed)."""
    plan, H, fronts, NP, NB, iperm = _plan_case(R, Cc, D, leaf, seed)
    n = R * Cc
    Sig = np.linalg.inv(H)
    scale = np.abs(Sig).max()
    rng = np.random.default_rng(seed)
    nsn = len(plan["first"]) - 1
    for _ in range(4):
        b = int(rng.integers(n))
        rows = [int(x) for x in rng.choice(n, size=3, replace=False)]
        got, fw, bw = _pruned_column(plan, fronts, NP, D, iperm, b, rows)
        ref = np.array([Sig[a * D:a * D + D, b * D:b * D + D] for a in rows])
        assert np.abs(got - ref).max() <= 1e-12 * scale
        if nsn > 1:
            assert len(fw | bw) < nsn or len(rows) * 2 >= nsn    # pruned: not the whole tree in general
        for s in fw:
            g2, *_ = _pruned_column(plan, fronts, NP, D, iperm, b, rows, skip_fw=s)
            assert np.abs(g2 - ref).max() > 1e-6 * scale, ("forward", s)
        for s in bw:
            g2, *_ = _pruned_column(plan, fronts, NP, D, iperm, b, rows, skip_bw=s)
            assert np.abs(g2 - ref).max() > 1e-6 * scale, ("backward", s)


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


def _pair_ref(blk, pairs):
    return np.array([np.block([[blk(a, a), blk(a, b)], [blk(b, a), blk(b, b)]]) for a, b in pairs])


def _set_ref(blk, ids):
    return np.block([[blk(a, b) for b in ids] for a in ids])


def _check_invariants(hg, fid, pairs, sel):
    """Invariants 1, 2 and 4 of the calls: diagonal sub-blocks equal marginalCovariances, edge pairs equal
    jointCovariances (bit for bit); the set is exactly symmetric, (a, b) / (b, a) are exact permutations, repeats are
    bit-identical."""
    d = hg.d
    ids_all = [int(i) for i in hg.vertices()[0]]
    _, M = hg.marginalCovariances(fixed_id=fid)
    at = {v: k for k, v in enumerate(ids_all)}
    Pp = hg.pairCovariances(pairs, fixed_id=fid)
    for k, (a, b) in enumerate(pairs):
        assert np.array_equal(Pp[k][:d, :d], M[at[int(a)]]) and np.array_equal(Pp[k][d:, d:], M[at[int(b)]])
    both = np.concatenate([pairs, pairs[:, ::-1]])
    Pb = hg.pairCovariances(both, fixed_id=fid)
    n = len(pairs)
    sw = np.concatenate([np.arange(d, 2 * d), np.arange(d)])
    assert np.array_equal(Pb[n:], Pb[:n][:, sw][:, :, sw])
    assert np.array_equal(Pb[:n], hg.pairCovariances(both, fixed_id=fid)[:n])
    ep = _edge_pairs(hg)
    assert np.array_equal(hg.pairCovariances(ep, fixed_id=fid), hg.jointCovariances(ep, fixed_id=fid))
    S = hg.jointMarginalCovariance(sel, fixed_id=fid)
    assert _off_diagonal_mirrored(S, d) and np.array_equal(S, hg.jointMarginalCovariance(sel, fixed_id=fid))
    for k, v in enumerate(sel):
        assert np.array_equal(S[k * d:k * d + d, k * d:k * d + d], M[at[int(v)]])
    return Pp, S


def _off_diagonal_mirrored(S, d):
    """Every off-diagonal D x D block is the exact transpose of its mirror (the diagonal blocks are the marginals as the
    selected inverse holds them, symmetric to rounding only)."""
    off = ~np.kron(np.eye(len(S) // d, dtype=bool), np.ones((d, d), bool))
    return np.array_equal(S[off], S.T[off])


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", SMALL)
def test_pair_and_set_blocks_equal_numpy_inverse_on_small_graphs(case, n, hip_ctx):
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, which, opts, *_ = util.load_golden(case)
    sub, w = util.prefix_graph(g, which, n)
    D = sub["pose_dim"]
    base = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx)
    sp = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx, useGLC=opts.algorithm == abi.ALG_GLC)
    st = sp.marginalizeNoOptimize(w, opts)
    assert st["n_bad_status"] == 0 and st["n_removed"] == len(w)
    kept = [int(i) for i in sp.vertices()[0]]
    worst = 0.0
    for hg, og in ((base, oracle_lib.OracleGraph.from_dict(sub)), (sp, _oracle_of(sp))):
        ids = [int(i) for i in hg.vertices()[0]]
        rng = np.random.default_rng(len(ids))
        for fid in (ids[0], kept[len(kept) // 2]):
            Sig = np.linalg.inv(og.information(fid))
            blk = _dense_blocks(Sig, ids, fid, D)
            scale = np.abs(Sig).max()
            far = _far_pairs(hg, 40, seed=fid)
            sel = np.array(sorted(rng.choice(ids, size=min(20, len(ids)), replace=False)), np.int32)
            Pp, S = _check_invariants(hg, fid, far, sel)
            err = np.abs(Pp - _pair_ref(blk, far)).max()
            err = max(err, np.abs(S - _set_ref(blk, sel)).max())
            v0 = ids[len(ids) // 3]
            star = np.array([(v0, v) for v in ids if v != v0], np.int32)
            Ps = hg.pairCovariances(star, fixed_id=fid)
            s = hg.last_covariance_stats
            assert s["columns"] == 1 and s["rhs_batches"] == 1 and s["solve_flops"] > 0 and s["solve_seconds"] > 0
            assert s["device_seconds"] > s["solve_seconds"] and s["supernodes"] > 0
            err = max(err, np.abs(Ps - _pair_ref(blk, star)).max())
            worst = max(worst, err / scale)
            assert err <= 1e-9 * scale, (case, hg is sp, fid, err / scale)
    print(f"{case}[{n}]: worst rel err {worst:.1e}, {len(kept)} kept")


@pytest.mark.gpu
def test_pair_and_set_blocks_equal_dense_covariance_on_sphere(hip_ctx):
    """sphere.g2o at full size (2 500 poses, 14 994 variables) against the dense covariance(): one vertex against all
    2 499 others, 2 000 random pairs, the joint marginal of 300 random vertices."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, *_ = util.load_golden("sphere_full_nfr_tree")
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    S = hg.covariance()
    ids = [int(i) for i in hg.vertices()[0]]
    blk = _dense_blocks(S, ids, ids[0], 6)
    scale = np.abs(S).max()
    v0 = ids[1234]
    star = np.array([(v0, v) for v in ids if v != v0], np.int32)
    Ps = hg.pairCovariances(star)
    s1 = dict(hg.last_covariance_stats)
    e1 = np.abs(Ps - _pair_ref(blk, star)).max() / scale
    rng = np.random.default_rng(7)
    rp = np.array([rng.choice(ids, size=2, replace=False) for _ in range(2000)], np.int32)
    Pr = hg.pairCovariances(rp)
    s2 = dict(hg.last_covariance_stats)
    e2 = np.abs(Pr - _pair_ref(blk, rp)).max() / scale
    sel = np.array(rng.choice(ids, size=300, replace=False), np.int32)
    J = hg.jointMarginalCovariance(sel)
    s3 = dict(hg.last_covariance_stats)
    e3 = np.abs(J - _set_ref(blk, sel)).max() / scale
    assert _off_diagonal_mirrored(J, 6)
    for name, s, e in (("one vs all", s1, e1), ("2000 random pairs", s2, e2), ("300-vertex set", s3, e3)):
        print(f"sphere full {name}: rel err {e:.1e}; {s['device_seconds'] * 1e3:.1f} ms device, solves {s['solve_seconds'] * 1e3:.1f} ms, "
              f"{s['columns']} columns in {s['rhs_batches']} batches, {s['solve_flops'] / 1e9:.1f} GFLOP")
    assert s1["columns"] == 1
    assert max(e1, e2, e3) <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere_full_glc_dense", "manhattan_cliquey_dense"])
def test_exactness_across_graphs_through_pair_covariances(name, hip_ctx):
    """GLC Dense and CliqueyDense keep the joint marginal of the kept vertices: for every vertex pair of every new n-ary
    edge, the sparsified graph's jointCovariances block equals the baseline's pairCovariances block (the two vertices
    share no edge in the baseline), without the dense covariance()."""
    base, sp = _exact_case(name, hip_ctx)
    pairs = _edge_pairs(sp, kinds={abi.EDGE_GLC, abi.EDGE_MULTI})
    assert len(pairs) > 0
    Js = sp.jointCovariances(pairs)
    Jb = base.pairCovariances(pairs, fixed_id=int(sp.vertices()[0][0]))
    s = base.last_covariance_stats
    err = np.abs(Js - Jb).max() / np.abs(Jb).max()
    print(f"{name}: {len(pairs)} n-ary pairs, rel err {err:.1e}; baseline {s['columns']} columns in {s['rhs_batches']} batches, "
          f"{s['device_seconds'] * 1e3:.1f} ms")
    assert s["columns"] > 0
    assert err <= 1e-9


_FORCED = r"""
import sys
import numpy as np
from sparsifyposegraph_amd import g2o_io
from sparsifyposegraph_amd.graph import GraphWrapperHIP
from sparsifyposegraph_amd.lib import Context
g = g2o_io.synth_sphere(100000, 400)
hg = GraphWrapperHIP.from_dict(g, ctx=Context(0))
pairs = np.ascontiguousarray(g["edge_ij"], np.int32)[::50]
J = hg.jointCovariances(pairs)
P = hg.pairCovariances(pairs)
s = hg.last_covariance_stats
np.savez(sys.argv[1], J=J, P=P, columns=s["columns"], batches=s["rhs_batches"], secs=s["device_seconds"])
"""


@pytest.mark.gpu
def test_pair_covariances_at_headline_size(hip_ctx, tmp_path):
    """synth_sphere(100000, 400) (600 k variables; the dense covariance() is SPG_ECAPACITY): one vertex against all
    99 999 others and 10 000 random pairs, each block symmetric positive definite, invariants 1 and 2 against the
    selected inverse; in a child process with SPG_COV_FORCE_SOLVE=1 the edge blocks by column solves agree with the
    selected inverse."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_sphere(100000, 400)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    ids = hg.vertices()[0]
    _, M = hg.marginalCovariances()
    at = {int(v): k for k, v in enumerate(ids)}
    v0 = int(ids[50000])
    star = np.array([(v0, int(v)) for v in ids if int(v) != v0], np.int32)
    Ps = hg.pairCovariances(star)
    s1 = dict(hg.last_covariance_stats)
    rng = np.random.default_rng(11)
    rp = np.array([rng.choice(100000, size=2, replace=False) for _ in range(10000)], np.int32)
    Pr = hg.pairCovariances(rp)
    s2 = dict(hg.last_covariance_stats)
    for P, pr in ((Ps, star), (Pr, rp)):
        ia, ib = np.array([at[int(a)] for a in pr[:, 0]]), np.array([at[int(b)] for b in pr[:, 1]])
        assert np.array_equal(P[:, :6, :6], M[ia]) and np.array_equal(P[:, 6:, 6:], M[ib])
        keep = (ia != 0) & (ib != 0)
        Q = P[keep]
        assert np.abs(Q - Q.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(Q).max()
        assert np.all(np.linalg.eigvalsh(0.5 * (Q + Q.transpose(0, 2, 1))) > 0)
    ep = np.ascontiguousarray(g["edge_ij"], np.int32)[::20]
    assert np.array_equal(hg.pairCovariances(ep), hg.jointCovariances(ep))
    for name, s in (("one vs all", s1), ("10 000 random pairs", s2)):
        print(f"100k {name}: {s['device_seconds']:.3f} s device, solves {s['solve_seconds']:.3f} s, {s['columns']} columns in "
              f"{s['rhs_batches']} batches, solve {s['solve_flops'] / 1e9:.1f} GFLOP, factor {s['factor_flops'] / 1e9:.1f} GFLOP, "
              f"selinv {s['selinv_flops'] / 1e9:.1f} GFLOP")
    assert s1["columns"] == 1
    out = str(tmp_path / "forced.npz")
    r = subprocess.run([sys.executable, "-c", _FORCED, out], env={**os.environ, "SPG_COV_FORCE_SOLVE": "1"}, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    f = np.load(out)
    err = np.abs(f["P"] - f["J"]).max() / np.abs(f["J"]).max()
    print(f"100k forced solves: {len(f['P'])} edge blocks, {int(f['columns'])} columns in {int(f['batches'])} batches, "
          f"{float(f['secs']):.3f} s device; rel err vs selected inverse {err:.1e}")
    assert int(f["columns"]) > 0 and err <= 1e-9


def _build_demo(tmp_path):
    exe = str(tmp_path / "pair_covariance_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pair_covariance_demo.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_pair_covariance_demo_compiles(tmp_path):
    out = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr


@pytest.mark.gpu
def test_cpp_facade_pair_covariances_match_python(tmp_path, hip_ctx):
    """tests/cpp/pair_covariance_demo.cpp calls the façade's pairCovariances / jointMarginalCovariance on a small sphere
    and prints the blocks; they equal the Python binding's bit for bit."""
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
    pairs = [(ids[0], ids[i]) for i in range(1, n)] + [(ids[i], ids[n - 1 - i]) for i in range(n // 2)]
    P = hg.pairCovariances(np.array(pairs, np.int32))
    S = hg.jointMarginalCovariance(np.array(ids[::7], np.int32))
    ref = np.concatenate([P.ravel(), S.ravel()])
    assert got.shape == ref.shape and np.array_equal(got, ref)
    assert "pair covariance ok" in out.stdout
