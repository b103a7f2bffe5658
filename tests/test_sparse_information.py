"""The Gauss-Newton information in block-CSR form (spg_graph_sparse_information, csrc/spg_bsr.inc + spg_bsr_pattern.hpp —
GraphWrapperG2O::sparseInformation, src/graph_wrapper_g2o.cpp:382-396) and the product H X (spg_graph_information_apply,
bsr_spmv_kernel).
CPU: the pattern on an injected context against a restatement in numpy from edges(), argument checking before the
backend, the C++ demo compiles. GPU: the expanded matrix equals spg_graph_information bit for bit on every shape, H X
against numpy within a derived bound and bitwise repeatable, the headline size, the C++ façade."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sparsifyposegraph_amd import abi, g2o_io
from sparsifyposegraph_amd.lib import SpgError
from tests import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")
_f64p, _i32p, _i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
EINVAL, ESTATE = abi.EINVAL, abi.ESTATE


# ------------------------------------------------------------------------------------------------------- graphs
def _pose(rng, d):
    if d == 3:
        return np.concatenate([rng.uniform(-3, 3, 2), rng.uniform(-1, 1, 1)])
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    return np.concatenate([rng.uniform(-3, 3, 3), q if q[3] >= 0 else -q])


def _spd_upper(rng, d):
    A = rng.standard_normal((d, d))
    return (A @ A.T + d * np.eye(d))[np.triu_indices(d)]


def _fill(hg, rng, ids, pairs):
    d = hg.d
    for v in ids:
        hg.addVertex(int(v), _pose(rng, d))
    for a, b in pairs:
        hg.addEdge(int(a), int(b), _pose(rng, d), _spd_upper(rng, d))


def _ring(hg, rng):
    """a ring of 12 with three chords"""
    ids = list(range(12))
    _fill(hg, rng, ids, [(i, (i + 1) % 12) for i in ids] + [(0, 5), (2, 9), (4, 10)])
    return -1


def _hub(hg, rng):
    """vertex 40 with 70 spokes (its row holds more than 64 blocks) and a short chain among the spokes; 70 block rows: no
    multiple of the 16 (SE2) or 8 (SE3) rows a workgroup of bsr_spmv_kernel takes"""
    ids = list(range(71))
    _fill(hg, rng, ids, [(40, v) for v in ids if v != 40] + [(1, 2), (2, 3), (68, 69)])
    return -1


def _awkward(hg, rng):
    """non-contiguous ids with the fixed vertex (41) in the middle of the range, two parallel edges on (10, 11), a self-loop
    on 77, and vertex 1001 whose only edge goes to the fixed vertex (its row holds the diagonal block only)"""
    ids = [3, 10, 11, 40, 41, 77, 200, 1000, 1001]
    _fill(hg, rng, ids, [(3, 10), (10, 11), (10, 11), (11, 40), (40, 41), (41, 77), (77, 200), (200, 1000), (3, 200), (77, 77), (1001, 41)])
    return 41


def _nary(hg, rng):
    """a chain of 9 with one 3-ary GLC edge and one MULTI edge of two correlated measurements over three vertices"""
    d = hg.d
    ids = [2, 4, 6, 8, 10, 12, 14, 16, 18]
    _fill(hg, rng, ids, [(ids[i], ids[i + 1]) for i in range(8)])
    q = 3
    meas = np.concatenate([_pose(rng, d)[:d] * 0.1 for _ in range(q)])        # reparametrised measurement: D numbers per vertex
    hg.addGLCEdge([4, 10, 16], meas, rng.standard_normal((d * q - d, d * q)))
    nm = 2
    ms = np.concatenate([_pose(rng, d) for _ in range(nm)])
    W = rng.standard_normal((d * nm, d * nm)) + 3 * np.eye(d * nm)
    hg.addMultiEdge([6, 12, 18], np.concatenate([[nm, 0, 1, 0, 2], ms, W.ravel()]))
    return -1


SHAPES = {"ring": _ring, "hub": _hub, "awkward": _awkward, "nary": _nary}
CASES = [(name, d) for name in SHAPES for d in (3, 6)]


def build(name, d, ctx):
    """the graph of a shape on `ctx` and the fixed id to use with it"""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    hg = GraphWrapperHIP(ctx=ctx, pose_dim=d)
    fixed = SHAPES[name](hg, np.random.default_rng(7 + d))
    return hg, fixed


def numpy_pattern(hg, fixed_id):
    """(ids, indptr, indices) restated from vertices() and edges(): the clique of every edge's free vertices plus the diagonal"""
    ids = np.sort(hg.vertices()[0])
    fid = int(ids[0]) if fixed_id < 0 else fixed_id
    free = ids[ids != fid]
    at = {int(v): i for i, v in enumerate(free)}
    nb = len(free)
    A = np.eye(nb, dtype=bool)
    e = hg.edges()
    for k in range(len(e["kind"])):
        vs = [at[int(v)] for v in e["vert_ids"][e["vert_off"][k]:e["vert_off"][k + 1]] if int(v) in at]
        for a in vs:
            for b in vs:
                A[a, b] = True
    indptr = np.concatenate([[0], np.cumsum(A.sum(1))]).astype(np.int64)
    return free.astype(np.int32), indptr, np.nonzero(A)[1].astype(np.int32)


def expand(indptr, indices, blocks, d):
    nb = len(indptr) - 1
    H = np.zeros((nb * d, nb * d))
    for i in range(nb):
        for k in range(indptr[i], indptr[i + 1]):
            j = indices[k]
            H[i * d:(i + 1) * d, j * d:(j + 1) * d] = blocks[k]
    return H


# ------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name,d", CASES)
def test_pattern_on_an_injected_context_equals_numpy(name, d):
    """No device: the pattern call answers on an injected context and equals the pattern restated from edges()."""
    hg, fixed = build(name, d, oracle_lib.injected_context())
    indptr, indices, blocks, ids = hg.sparseInformation(fixed, values=False)
    assert blocks is None
    rid, rptr, rind = numpy_pattern(hg, fixed)
    nb = len(rid)
    assert np.array_equal(ids, rid) and np.all(np.diff(ids) > 0) and (fixed if fixed >= 0 else int(hg.vertices()[0].min())) not in ids
    assert indptr[0] == 0 and np.all(np.diff(indptr) >= 1) and len(indptr) == nb + 1
    assert indptr[-1] == len(indices) == len(rind)
    assert np.array_equal(indptr, rptr) and np.array_equal(indices, rind)
    A = np.zeros((nb, nb), bool)
    for i in range(nb):
        cols = indices[indptr[i]:indptr[i + 1]]
        assert np.all(np.diff(cols) > 0) and i in cols
        A[i, cols] = True
    assert np.array_equal(A, A.T)
    if name == "awkward":
        row = list(ids).index(1001)
        assert indptr[row + 1] - indptr[row] == 1            # only edge goes to the fixed vertex: the diagonal block alone
        r10 = list(ids).index(10)
        assert list(indices[indptr[r10]:indptr[r10 + 1]]).count(list(ids).index(11)) == 1    # parallel edges share a block
        r77 = list(ids).index(77)
        assert list(ids[indices[indptr[r77]:indptr[r77 + 1]]]) == [77, 200]                  # the self-loop adds nothing
    if name == "hub":
        row = list(ids).index(40)
        assert indptr[row + 1] - indptr[row] == 70 > 64


def test_arguments_are_checked_before_the_backend():
    """On an injected (CPU) context: the size query and the pattern answer; an unknown fixed id and nrhs <= 0 are
    SPG_EINVAL, a too small cap_blocks writes nothing (and returns the count, the two-call idiom), value calls are
    SPG_ESTATE (no CPU fallback) and write nothing either."""
    ictx = oracle_lib.injected_context()
    hg, _ = build("ring", 3, ictx)
    L = hg.L
    nnzb = L.spg_graph_sparse_information(hg.h, -1, None, None, None, 0, None)
    assert nnzb == 11 + 2 * (10 + 2)      # 11 free vertices; ring without vertex 0: 10 edges, chords without (0, 5): 2
    ptr, col, ids = np.full(12, -7, np.int64), np.full(nnzb, -7, np.int32), np.full(11, -7, np.int32)
    val = np.full(nnzb * 9, -7.0)
    p64, p32, pf = (lambda a: a.ctypes.data_as(_i64p)), (lambda a: a.ctypes.data_as(_i32p)), (lambda a: a.ctypes.data_as(_f64p))
    assert L.spg_graph_sparse_information(hg.h, -1, p64(ptr), p32(col), None, nnzb - 1, p32(ids)) == nnzb
    assert np.all(ptr == -7) and np.all(col == -7) and np.all(ids == -7)
    assert L.spg_graph_sparse_information(hg.h, -1, p64(ptr), p32(col), pf(val), nnzb, p32(ids)) == ESTATE
    assert "HIP backend" in L.spg_last_error(ictx.h).decode()
    assert np.all(ptr == -7) and np.all(col == -7) and np.all(ids == -7) and np.all(val == -7.0)
    assert L.spg_graph_sparse_information(hg.h, 999999, None, None, None, 0, None) == EINVAL
    assert "fixed vertex" in L.spg_last_error(ictx.h).decode()
    assert L.spg_graph_sparse_information(hg.h, -1, p64(ptr), p32(col), None, -1, None) == EINVAL
    assert L.spg_graph_sparse_information(hg.h, -1, p64(ptr), p32(col), None, nnzb, None) == nnzb      # ids may be NULL
    assert ptr[0] == 0 and ptr[-1] == nnzb and np.all(ids == -7)
    x, y = np.ones(33), np.full(33, -7.0)
    assert L.spg_graph_information_apply(hg.h, -1, pf(x), 0, pf(y)) == EINVAL
    assert L.spg_graph_information_apply(hg.h, -1, pf(x), -3, pf(y)) == EINVAL
    assert L.spg_graph_information_apply(hg.h, -1, None, 1, pf(y)) == EINVAL
    assert L.spg_graph_information_apply(hg.h, 999999, pf(x), 1, pf(y)) == EINVAL
    assert L.spg_graph_information_apply(hg.h, -1, pf(x), 1, pf(y)) == ESTATE
    assert np.all(y == -7.0)
    with pytest.raises(SpgError, match="HIP backend"):
        hg.sparseInformation()
    with pytest.raises(SpgError, match="HIP backend"):
        hg.informationApply(x)
    with pytest.raises(SpgError, match="fixed vertex"):
        hg.sparseInformation(fixed_id=999999, values=False)
    with pytest.raises(ValueError):
        hg.informationApply(np.ones(32))
    # the solver enum and the PCG parameters live on the context
    assert L.spg_ctx_set_linear_solver(ictx.h, abi.SOLVER_PCG) == 0 and L.spg_ctx_set_linear_solver(ictx.h, 4) == EINVAL
    ictx.set_linear_solver(abi.SOLVER_AUTO)
    ictx.set_pcg(1e-8, 100)
    ictx.set_pcg()
    assert ictx.pcg_stats() == {"solves": 0, "unconverged": 0, "iterations": 0, "last_rel_residual": 0.0, "solve_seconds": 0.0}


def _build_demo(tmp_path):
    exe = str(tmp_path / "sparse_information_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "sparse_information_demo.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_sparse_information_demo_compiles(tmp_path):
    out = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr


# ------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def device_cases(hip_ctx):
    """every shape once: the graph, its fixed id, the dense information and the block-CSR export"""
    out = {}
    for name, d in CASES:
        hg, fixed = build(name, d, hip_ctx)
        out[name, d] = (hg, fixed, hg.information(fixed), hg.sparseInformation(fixed))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,d", CASES)
def test_expanded_blocks_equal_the_dense_information_bit_for_bit(name, d, device_cases):
    """Same kernel body, same accumulation order, only the sink differs: rtol = 0, atol = 0. The pattern equals the numpy
    restatement, blocks outside it are exactly zero in the dense matrix, and block (u, v) is the transpose of (v, u)."""
    hg, fixed, H, (indptr, indices, blocks, ids) = device_cases[name, d]
    rid, rptr, rind = numpy_pattern(hg, fixed)
    assert np.array_equal(ids, rid) and np.array_equal(indptr, rptr) and np.array_equal(indices, rind)
    assert blocks.shape == (len(indices), d, d) and H.shape == (len(ids) * d,) * 2
    E = expand(indptr, indices, blocks, d)
    print(f"{name} SE{2 if d == 3 else 3}: {len(ids)} block rows, {len(indices)} blocks, max |BSR - dense| = {np.abs(E - H).max():.3g}")
    assert np.array_equal(E, H)
    nb = len(ids)
    inside = np.zeros((nb, nb), bool)
    for i in range(nb):
        inside[i, indices[indptr[i]:indptr[i + 1]]] = True
    assert np.all(H[~np.kron(inside, np.ones((d, d), bool))] == 0.0)
    at = {(i, int(indices[k])): k for i in range(nb) for k in range(indptr[i], indptr[i + 1])}
    for (i, j), k in at.items():
        assert np.array_equal(blocks[k], blocks[at[j, i]].T), (i, j)
    assert np.all(np.linalg.eigvalsh(E) > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("nrhs", [1, 5])
@pytest.mark.parametrize("name,d", CASES)
def test_information_apply_equals_numpy_within_the_derived_bound(name, d, nrhs, device_cases):
    """|y - H x| <= 8 (D blocks in the row) 2^-53 (|H| |x|) componentwise: a row's sum has D * blocks terms, each side
    (the kernel's slot-wise sums and numpy's) commits at most that many roundings of relative size 2^-53, the factor 8
    leaves room for the order of the partial sums. Two runs give the same bits."""
    hg, fixed, H, (indptr, indices, blocks, ids) = device_cases[name, d]
    n = H.shape[0]
    X = np.random.default_rng(5).standard_normal((nrhs, n))
    Y = hg.informationApply(X if nrhs > 1 else X[0], fixed).reshape(nrhs, n)
    ref = X @ H.T
    bound = 8.0 * np.repeat(d * np.diff(indptr), d) * 2.0 ** -53 * (np.abs(X) @ np.abs(H).T)
    err = np.abs(Y - ref)
    print(f"{name} SE{2 if d == 3 else 3} nrhs={nrhs}: worst |y - ref| / bound = {(err / bound).max():.3g}")
    assert np.all(err <= bound)
    again = hg.informationApply(X if nrhs > 1 else X[0], fixed).reshape(nrhs, n)
    assert np.array_equal(Y, again)


@pytest.mark.gpu
def test_headline_size(hip_ctx):
    """synth_sphere(100000, 400): 599 994 variables. The dense information() would be 2.9 TB, ten times the device's
    288 GB, so the call cannot deliver it; sparseInformation() does. nnzb equals the numpy pattern count, and H applied
    to a unit block vector reproduces that block column."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_sphere(100000, 400)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    d = 6
    n = hg.L.spg_graph_information(hg.h, -1, None, 0)
    assert n == d * 99999 and n * n * 8 > 9 * 288e9
    indptr, indices, blocks, ids = hg.sparseInformation()
    ij = np.asarray(g["edge_ij"])
    ij = ij[(ij[:, 0] != 0) & (ij[:, 1] != 0) & (ij[:, 0] != ij[:, 1])]
    pairs = np.unique(np.sort(ij, axis=1), axis=0)
    assert len(indices) == indptr[-1] == 99999 + 2 * len(pairs)
    assert np.array_equal(ids, np.arange(1, 100000))
    print(f"100k: {len(indices)} blocks, {blocks.nbytes / 1e6:.0f} MB of values")
    col = 50000
    X = np.zeros((d, n))
    X[np.arange(d), col * d + np.arange(d)] = 1.0
    Y = hg.informationApply(X)
    want = np.zeros((n, d))
    rows = np.repeat(np.arange(99999), np.diff(indptr))
    for k in np.nonzero(indices == col)[0]:
        want[rows[k] * d:(rows[k] + 1) * d] = blocks[k]
    assert np.array_equal(Y.T, want)


@pytest.mark.gpu
def test_cpp_facade_sparse_information(tmp_path):
    """tests/cpp/sparse_information_demo.cpp: sparseInformation / informationApply / the PCG selection through the façade"""
    path = str(tmp_path / "s200.g2o")
    g2o_io.write_g2o(path, g2o_io.synth_sphere(n_poses=200, ring=20))
    out = subprocess.run([_build_demo(tmp_path), path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sparse information ok" in out.stdout
