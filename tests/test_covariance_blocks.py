"""Per-pose marginal covariances, joint covariances of edge pairs and the per-vertex marginal KLD from the selected inverse
of the sparse factor (spg_graph_marginal_covariances / _joint_covariances / _marginal_kld, csrc/spg_sparse.inc:
sp_sigma_blocks_kernel, sp_marginal_kld_kernel) — GraphWrapperISAM::covariance (src/graph_wrapper_isam.cpp:259-262)
reads marginal blocks from iSAM's factor the same way.
CPU: argument checking before the backend, the size queries, and a numpy restatement of the plan without marginalised
blocks (every pair of an n-ary edge is found in one front, the selected inverse over all supernodes is inv(H)).
GPU: exact values against numpy on small graphs (before and after marginalisation), against the dense covariance() on
sphere.g2o at full size, the exactness of GLC Dense / CliqueyDense seen pose by pose, the headline size, the C++ façade."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sparsifyposegraph_amd import abi, g2o_io
from sparsifyposegraph_amd.lib import SpgError, sparse_plan
from tests import oracle_lib, util
from tests.test_sparse_plan import lattice, multifrontal, random_spd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")
_f64p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
EINVAL, ESTATE = -1, -7


def _small(n=30):
    g, which, *_ = util.load_golden("intel_nfr_tree_sp3")
    sub, _ = util.prefix_graph(g, which, n)
    return sub


def _non_adjacent_pair(sub):
    adj = {(int(a), int(b)) for a, b in sub["edge_ij"]}
    ids = [int(i) for i in sub["ids"]]
    for a in ids:
        for b in ids:
            if a != b and (a, b) not in adj and (b, a) not in adj:
                return a, b
    raise AssertionError("no non-adjacent pair")


# ------------------------------------------------------------------------------------------------------- CPU
def test_covariance_calls_check_arguments_before_the_backend():
    """On an injected (CPU) context: unknown ids / fixed vertex and pairs without a common edge are SPG_EINVAL, the size
    queries answer, and a call that would compute is SPG_ESTATE (no CPU fallback)."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    sub = _small()
    ictx = oracle_lib.injected_context()
    a, b = GraphWrapperHIP.from_dict(sub, ctx=ictx), GraphWrapperHIP.from_dict(sub, ctx=ictx)
    L, D, nv = a.L, 3, len(sub["ids"])
    ids = np.ascontiguousarray(sub["ids"][:5], np.int32)
    e0 = [int(x) for x in sub["edge_ij"][0]]
    pairs = np.array([e0, [e0[1], e0[0]]], np.int32)
    buf = np.zeros(4096)
    f = lambda x: x.ctypes.data_as(_f64p)  # noqa: E731
    i = lambda x: x.ctypes.data_as(_i32p)  # noqa: E731
    # size queries
    assert L.spg_graph_marginal_covariances(a.h, -1, None, 0, None, 0, None) == nv * D * D
    assert L.spg_graph_marginal_covariances(a.h, -1, i(ids), 5, None, 0, None) == 5 * D * D
    assert L.spg_graph_marginal_covariances(a.h, -1, i(ids), 5, f(buf), 5 * D * D - 1, None) == 5 * D * D
    assert L.spg_graph_joint_covariances(a.h, -1, i(pairs), 2, None, 0, None) == 2 * (2 * D) ** 2
    assert L.spg_graph_marginal_kld(a.h, b.h, -1, None, None, 0, None) == nv - 1
    # no HIP backend
    st = abi.CovStats()
    assert L.spg_graph_marginal_covariances(a.h, -1, i(ids), 5, f(buf), buf.size, C.byref(st)) == ESTATE
    assert L.spg_graph_joint_covariances(a.h, -1, i(pairs), 2, f(buf), buf.size, C.byref(st)) == ESTATE
    kid, kv = np.zeros(nv, np.int32), np.zeros(nv)
    assert L.spg_graph_marginal_kld(a.h, b.h, -1, i(kid), f(kv), nv, C.byref(st)) == ESTATE
    # invalid arguments, answered before the backend
    bad_ids = np.array([int(ids[0]), 999999], np.int32)
    assert L.spg_graph_marginal_covariances(a.h, -1, i(bad_ids), 2, None, 0, None) == EINVAL
    assert L.spg_graph_marginal_covariances(a.h, 999999, i(ids), 5, None, 0, None) == EINVAL
    assert L.spg_graph_joint_covariances(a.h, 999999, i(pairs), 2, None, 0, None) == EINVAL
    assert L.spg_graph_marginal_kld(a.h, b.h, 999999, None, None, 0, None) == EINVAL
    na = np.array(_non_adjacent_pair(sub), np.int32)
    assert L.spg_graph_joint_covariances(a.h, -1, i(na), 1, None, 0, None) == EINVAL
    assert f"({na[0]}, {na[1]})" in L.spg_last_error(ictx.h).decode()
    same = np.array([e0[0], e0[0]], np.int32)
    assert L.spg_graph_joint_covariances(a.h, -1, i(same), 1, None, 0, None) == EINVAL
    # other must be a subset of the baseline
    small = GraphWrapperHIP.from_dict(_small(20), ctx=ictx)
    assert L.spg_graph_marginal_kld(small.h, a.h, -1, None, None, 0, None) == EINVAL
    # the Python layer raises for each
    with pytest.raises(SpgError, match="HIP backend"):
        a.marginalCovariances()
    with pytest.raises(SpgError, match="HIP backend"):
        a.jointCovariances(pairs)
    with pytest.raises(SpgError, match="HIP backend"):
        a.marginalKullbackLeibler(b)
    with pytest.raises(SpgError, match="not in the graph"):
        a.marginalCovariances(bad_ids)
    with pytest.raises(SpgError, match="fixed vertex"):
        a.marginalCovariances(ids, fixed_id=999999)
    with pytest.raises(SpgError, match="share no live edge"):
        a.jointCovariances([na])
    with pytest.raises(SpgError, match="fixed vertex"):
        a.marginalKullbackLeibler(b, fixed_id=999999)
    with pytest.raises(SpgError, match="lacks"):
        small.marginalKullbackLeibler(a)


def _cliques(n, k, seed):
    rng = np.random.default_rng(seed)
    return [sorted(int(x) for x in rng.choice(n, size=int(rng.integers(3, 6)), replace=False)) for _ in range(k)]


@pytest.mark.parametrize("R,Cc,D,leaf", [(9, 11, 3, 6), (7, 8, 6, 5), (3, 25, 3, 1000)])
def test_selected_inverse_over_the_graphs_own_plan(R, Cc, D, leaf):
    """The plan without marginalised blocks (is_marg = NULL): the selected inverse of every supernode equals inv(H) on every
    real front position, and every vertex pair of every n-ary edge (cliques of 3 to 5 vertices) is found by the lookup rule
    of sp_sigma_blocks_kernel / FrontSink::locate: the later-eliminated vertex is a pivot of the earlier one's supernode or
    one of its boundary rows; a boundary pair is read from the upper-right block (Sigma_SB, transposed)."""
    _, _, pairs = lattice(R, Cc, 3, seed=R)
    n = R * Cc
    cl = _cliques(n, 6, seed=D + R)
    allp = set(pairs)
    for c in cl:
        allp.update((a, b) for x, a in enumerate(c) for b in c[x + 1:])
    adj = [[] for _ in range(n)]
    for a, b in allp:
        adj[a].append(b)
        adj[b].append(a)
    ptr = np.zeros(n + 1, np.int32)
    ptr[1:] = np.cumsum([len(x) for x in adj])
    adjv = np.array([u for x in adj for u in sorted(x)], np.int32)
    plan = sparse_plan(ptr, adjv, D, leaf=leaf)
    assert plan["n_marg_supernodes"] == 0
    H = random_spd(n, D, sorted(allp), seed=5)
    fronts, logdiag, NP, NB, iperm, sig = multifrontal(plan, H, D, selinv_from=0)
    Sig = np.linalg.inv(H)
    first, rowptr, rows, perm = plan["first"], plan["rowptr"], plan["rows"], plan["perm"]
    nsn = len(first) - 1
    assert sorted(sig) == list(range(nsn))
    worst = 0.0
    for s in range(nsn):
        cols = list(range(first[s], first[s + 1]))
        loc = [(q, D * i) for i, q in enumerate(cols)] + [(q, NP[s] + D * i) for i, q in enumerate(rows[rowptr[s]:rowptr[s + 1]])]
        for q1, o1 in loc:
            for q2, o2 in loc:
                ref = Sig[perm[q1] * D:perm[q1] * D + D, perm[q2] * D:perm[q2] * D + D]
                worst = max(worst, np.abs(sig[s][o1:o1 + D, o2:o2 + D] - ref).max())
    assert worst <= 1e-9 * np.abs(Sig).max()
    sn_of = np.repeat(np.arange(nsn), np.diff(first))

    def read(pa, pb):   # Sigma block (block positions pa, pb) by the kernel's rule
        if pa < pb:
            return read(pb, pa).T
        pv, pu = pa, pb
        s = sn_of[pu]
        col = D * (pu - first[s])
        if pv < first[s + 1]:
            r0 = D * (pv - first[s])
            return sig[s][r0:r0 + D, col:col + D]
        brow = list(rows[rowptr[s]:rowptr[s + 1]])
        assert pv in brow, "pair outside the front"
        r0 = NP[s] + D * brow.index(pv)
        return sig[s][col:col + D, r0:r0 + D].T      # Sigma_SB is stored [column][boundary row]
    worst = 0.0
    for c in cl:
        for a in c:
            for b in c:
                got = read(iperm[a], iperm[b])
                worst = max(worst, np.abs(got - Sig[a * D:a * D + D, b * D:b * D + D]).max())
    assert worst <= 1e-9 * np.abs(Sig).max()


# ------------------------------------------------------------------------------------------------------- GPU
def _oracle_of(hg):
    """Oracle graph holding exactly the vertices and edges of a product graph (n-ary edges included)."""
    ids, poses = hg.vertices()
    o = oracle_lib.OracleGraph(hg.d)
    for i, p in zip(ids, poses):
        o.L.spgref_graph_add_vertex(o.h, int(i), np.ascontiguousarray(p, np.float64).ctypes.data_as(_f64p))
    e = hg.edges()
    for k in range(len(e["kind"])):
        vs = e["vert_ids"][e["vert_off"][k]:e["vert_off"][k + 1]]
        assert o.add_edge(int(e["kind"][k]), vs, e["data"][e["data_off"][k]:e["data_off"][k + 1]]) == 0
    return o


def _edge_pairs(hg, kinds=None):
    e = hg.edges()
    out = set()
    for k in range(len(e["kind"])):
        if kinds is not None and int(e["kind"][k]) not in kinds:
            continue
        vs = [int(v) for v in e["vert_ids"][e["vert_off"][k]:e["vert_off"][k + 1]]]
        out.update((a, b) for x, a in enumerate(vs) for b in vs[x + 1:])
    return np.array(sorted(out), np.int32).reshape(-1, 2)


def _dense_blocks(Sig, ids, fid, D):
    """Sigma with zero rows / columns for the fixed vertex, as a function of an id pair."""
    free = [int(i) for i in ids if int(i) != fid]
    at = {v: k for k, v in enumerate(free)}

    def blk(a, b):
        if a == fid or b == fid:
            return np.zeros((D, D))
        return Sig[at[a] * D:at[a] * D + D, at[b] * D:at[b] * D + D]
    return blk


def _ref_kld(Sx, Sy, diff):
    """kullbackLeiblerDivergence(diff, Sx^-1, Sy^-1, InformationInformation) (src/utils.cpp:70-97) literally."""
    infox, maty = np.linalg.inv(Sx), np.linalg.inv(Sy)
    logdetx = np.linalg.slogdet(infox)[1]
    logdety = -np.linalg.slogdet(maty)[1]
    inner = np.trace(np.linalg.solve(maty, infox))
    return 0.5 * (inner + diff @ infox @ diff - logdetx - logdety - len(diff))


SMALL = [("intel_nfr_tree_sp3", 600), ("sphere_nfr_tree", 500), ("manhattan_glc_tree", 600), ("sphere_glc_tree", 400),
         ("sphere_cliquey_subgraph", 400)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", SMALL)
def test_blocks_equal_numpy_inverse_on_small_graphs(case, n, hip_ctx):
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, which, opts, *_ = util.load_golden(case)
    sub, w = util.prefix_graph(g, which, n)
    D = sub["pose_dim"]
    base = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx)
    sp = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx, useGLC=opts.algorithm == abi.ALG_GLC)
    st = sp.marginalizeNoOptimize(w, opts)
    assert st["n_bad_status"] == 0 and st["n_removed"] == len(w)
    kinds = set(int(k) for k in sp.edges()["kind"])
    assert kinds != {abi.EDGE_BINARY} or opts.algorithm == abi.ALG_NFR and opts.topology == abi.TOPO_TREE
    kept = [int(i) for i in sp.vertices()[0]]
    worst = {}
    for hg, og in ((base, oracle_lib.OracleGraph.from_dict(sub)), (sp, _oracle_of(sp))):
        ids = [int(i) for i in hg.vertices()[0]]
        for fid in (ids[0], kept[len(kept) // 2]):
            Sig = np.linalg.inv(og.information(fid))
            blk = _dense_blocks(Sig, ids, fid, D)
            scale = np.abs(Sig).max()
            got_ids, M = hg.marginalCovariances(fixed_id=-1 if fid == ids[0] else fid)
            assert list(got_ids) == ids and M.shape == (len(ids), D, D)
            err = max(np.abs(M[k] - blk(v, v)).max() for k, v in enumerate(ids))
            assert not M[ids.index(fid)].any()
            sel = np.array(ids[::7], np.int32)
            _, Ms = hg.marginalCovariances(sel, fixed_id=fid)
            assert np.array_equal(Ms, M[::7])
            pairs = _edge_pairs(hg)
            J = hg.jointCovariances(pairs, fixed_id=fid)
            for k, (a, b) in enumerate(pairs):
                ref = np.block([[blk(a, a), blk(a, b)], [blk(b, a), blk(b, b)]])
                err = max(err, np.abs(J[k] - ref).max())
            s = hg.last_covariance_stats
            assert s["supernodes"] > 0 and s["factor_flops"] > 0 and s["selinv_flops"] > 0 and s["device_seconds"] > 0
            worst[(hg is sp, fid)] = err / scale
            assert err <= 1e-9 * scale, (case, hg is sp, fid, err / scale)
    # per-vertex marginal KLD of the sparsified graph against the baseline, both gauges
    fid = kept[len(kept) // 2]
    if D == 3:   # move one kept vertex of the sparsified graph: a Mahalanobis term (estimateDifference, SE2)
        vid = kept[len(kept) // 3]
        p = sp.vertices()[1][kept.index(vid)].copy()
        sp.setEstimate(vid, p + [0.01, -0.02, 0.0])
    og_b, og_s = oracle_lib.OracleGraph.from_dict(sub), _oracle_of(sp)
    ids_b = [int(i) for i in base.vertices()[0]]
    pb, ps = base.vertices()[1], sp.vertices()[1]
    for f in (-1, fid):
        fx = ids_b[0] if f < 0 else f
        Sy = _dense_blocks(np.linalg.inv(og_b.information(fx)), ids_b, fx, D)
        Sx = _dense_blocks(np.linalg.inv(og_s.information(fx)), kept, fx, D)
        got_ids, got = base.marginalKullbackLeibler(sp, fixed_id=f)
        assert list(got_ids) == [v for v in kept if v != fx]
        for v, k in zip(got_ids, got):
            diff = np.zeros(D)
            if D == 3:
                diff = pb[ids_b.index(v)] - ps[kept.index(v)]
                diff[2] = (diff[2] + np.pi) % (2 * np.pi) - np.pi
            elif np.abs(pb[ids_b.index(v)] - ps[kept.index(v)]).max() > 0:
                raise AssertionError("SE3 estimates moved")
            ref = _ref_kld(Sx(v, v), Sy(v, v), diff)
            assert abs(k - ref) <= 1e-9 * max(1.0, abs(ref)), (v, k, ref)
    print(f"{case}[{n}]: worst rel err {max(worst.values()):.1e}, {len(kept)} kept, kinds {sorted(kinds)}")


@pytest.mark.gpu
def test_blocks_equal_dense_covariance_on_sphere(hip_ctx):
    """sphere.g2o at full size (2 500 poses, 14 994 variables): every marginal block and every edge's joint block against
    the blocks of the dense covariance() (blocked Cholesky, triangular inverse, L^-T L^-1)."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, *_ = util.load_golden("sphere_full_nfr_tree")
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    S = hg.covariance()
    assert S.shape == (14994, 14994)
    ids = [int(i) for i in hg.vertices()[0]]
    blk = _dense_blocks(S, ids, ids[0], 6)
    scale = np.abs(S).max()
    _, M = hg.marginalCovariances()
    mst = dict(hg.last_covariance_stats)
    err = max(np.abs(M[k] - blk(v, v)).max() for k, v in enumerate(ids))
    pairs = _edge_pairs(hg)
    J = hg.jointCovariances(pairs)
    for k, (a, b) in enumerate(pairs):
        err = max(err, np.abs(J[k] - np.block([[blk(a, a), blk(a, b)], [blk(b, a), blk(b, b)]])).max())
    print(f"sphere full: {len(ids)} marginal + {len(pairs)} joint blocks, worst rel err vs dense {err / scale:.1e}; "
          f"{mst['device_seconds'] * 1e3:.1f} ms, {mst['supernodes']} supernodes")
    assert err <= 1e-9 * scale


def _exact_case(name, hip_ctx):
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    if name == "sphere_full_glc_dense":
        src, alg, topo, *_ = util.load_digest(name)
        g, which, *_ = util.load_golden(src)
        opts = abi.make_options(6, alg, topo)
    else:
        g, which, opts, *_ = util.load_golden(name)
    base = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    sp = GraphWrapperHIP.from_dict(g, ctx=hip_ctx, useGLC=opts.algorithm == abi.ALG_GLC)
    st = sp.marginalizeNoOptimize(which, opts)
    assert st["n_bad_status"] == 0 and st["n_removed"] == len(which)
    return base, sp


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere_full_glc_dense", "manhattan_cliquey_dense"])
def test_exact_marginalisation_keeps_every_marginal(name, hip_ctx):
    """GLC Dense and CliqueyDense reproduce the marginal of the kept vertices (global KLD ~ 0 by construction): pose by pose
    the sparsified graph's marginal covariances and the joint blocks of every new n-ary edge equal the baseline's, and
    every per-vertex KLD vanishes. The two vertices of a pair of a new edge share no edge in the baseline: its side of the
    joint blocks comes from the dense covariance()."""
    base, sp = _exact_case(name, hip_ctx)
    kept = sp.vertices()[0]
    _, Mb = base.marginalCovariances(kept)
    _, Ms = sp.marginalCovariances(kept)
    scale = np.abs(Mb).max()
    err_m = np.abs(Ms - Mb).max() / scale
    pairs = _edge_pairs(sp, kinds={abi.EDGE_GLC, abi.EDGE_MULTI})
    assert len(pairs) > 0
    Js = sp.jointCovariances(pairs)
    blk = _dense_blocks(base.covariance(), [int(i) for i in base.vertices()[0]], int(kept[0]), sp.d)
    Jb = np.array([np.block([[blk(a, a), blk(a, b)], [blk(b, a), blk(b, b)]]) for a, b in pairs])
    err_j = np.abs(Js - Jb).max() / np.abs(Jb).max()
    ids, kld = base.marginalKullbackLeibler(sp)
    t = base.last_covariance_stats
    assert np.array_equal(ids, kept[1:])
    print(f"{name}: {len(kept)} kept, {len(pairs)} n-ary pairs; marginals rel err {err_m:.1e}, joint {err_j:.1e}, "
          f"max per-vertex KLD {kld.max():.1e} ({t['device_seconds'] * 1e3:.1f} ms for both graphs)")
    assert err_m <= 1e-9 and err_j <= 1e-9
    assert np.all(np.abs(kld) <= 1e-9)


@pytest.mark.gpu
def test_covariance_blocks_at_headline_size(hip_ctx):
    """BASELINE config 5's graph (100 000 SE3 poses): all marginal blocks of the baseline, the joint block of every edge and
    the 50 001 per-vertex KLDs of the NFR Tree sparsified graph — sizes the dense covariance() cannot hold."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_sphere(100000, 400)
    which = np.array([i for i in range(4, 100000) if i % 2], np.int32)
    base = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    sp = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    st = sp.marginalizeNoOptimize(which, abi.make_options(6))
    assert st["n_bad_status"] == 0 and st["n_removed"] == len(which)
    ids, M = base.marginalCovariances()
    mst = dict(base.last_covariance_stats)
    assert len(ids) == 100000 and not M[0].any()
    assert np.abs(M - M.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(M).max()
    assert np.all(np.linalg.eigvalsh(M[1:]) > 0)
    pairs = np.ascontiguousarray(g["edge_ij"], np.int32)
    J = base.jointCovariances(pairs)
    jst = dict(base.last_covariance_stats)
    at = {int(v): k for k, v in enumerate(ids)}
    ia, ib = np.array([at[int(a)] for a in pairs[:, 0]]), np.array([at[int(b)] for b in pairs[:, 1]])
    assert np.array_equal(J[:, :6, :6], M[ia]) and np.array_equal(J[:, 6:, 6:], M[ib])
    kid, kld = base.marginalKullbackLeibler(sp)
    kst = dict(base.last_covariance_stats)
    assert len(kid) == 100000 - len(which) - 1 and np.all(np.isfinite(kld)) and kld.min() >= -1e-12
    for name, s in (("marginals", mst), ("joint", jst), ("marginal KLD", kst)):
        print(f"100k {name}: {s['device_seconds']:.3f} s on the device, {s['supernodes']} supernodes, {s['front_bytes'] / 1e9:.2f} GB, "
              f"factor {s['factor_flops'] / 1e9:.1f} GFLOP, selinv {s['selinv_flops'] / 1e9:.1f} GFLOP")
    print(f"100k per-vertex KLD: sum {kld.sum():.6g}, max {kld.max():.3g} at id {kid[int(np.argmax(kld))]}")


def _build_demo(tmp_path):
    exe = str(tmp_path / "covariance_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "covariance_demo.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_covariance_demo_compiles(tmp_path):
    out = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr


@pytest.mark.gpu
def test_cpp_facade_covariances_match_python(tmp_path, hip_ctx):
    """tests/cpp/covariance_demo.cpp calls the façade's marginalCovariances / jointCovariances / marginalKullbackLeibler on a
    small sphere (before and after NFR Tree) and prints the blocks; they equal the Python binding's bit for bit."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_sphere(n_poses=200, ring=20)
    path = str(tmp_path / "s200.g2o")
    g2o_io.write_g2o(path, g)
    out = subprocess.run([_build_demo(tmp_path), path, str(tmp_path / "cpp.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.loadtxt(str(tmp_path / "cpp.txt"))
    base = GraphWrapperHIP.load(path, ctx=hip_ctx)
    sp = GraphWrapperHIP.load(path, ctx=hip_ctx)
    sp.marginalizeNoOptimize(np.array([i for i in range(4, 200) if i % 2], np.int32), abi.make_options(6))
    _, M = sp.marginalCovariances()
    J = sp.jointCovariances(_edge_pairs(sp))
    _, k = base.marginalKullbackLeibler(sp)
    ref = np.concatenate([M.ravel(), J.ravel(), k])
    assert got.shape == ref.shape and np.array_equal(got, ref)
    assert "covariance ok" in out.stdout
