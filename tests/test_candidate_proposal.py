"""Loop-closure candidates proposed on the device (spg_graph_propose_candidates, csrc/spg_propose.inc) against the plain
numpy rule of tests/propose_ref.py.
CPU: the reference against independent restatements (the kept set as a union of per-vertex nearest-neighbour picks, the cap,
m = 0, the grid count), the fixtures of the GPU tests free of threshold ties, the argument contract on an injected backend,
the ABI and the bindings, the C++ demo compiles.
GPU, SE2 and SE3, n <= 2 000: lattices on cell borders (one unjittered, bit for bit), 300 poses in one cell, two clusters 10^6
apart, n = 1 / 2 / no pair, marginalised graphs (non-contiguous ids, n-ary edges in rule 4), query lists, max_angle and
min_id_gap, a forced small cell table in a child process; the range gate on the small graphs of the covariance tests in
both gauges, and on a drifted loop.

What the stage-A tests assert: ij equals the reference exactly; two calls return identical bits; pairs_tested equals
propose_ref.cells_tested (the search is a grid search); |dist - ref| <= 16 eps max(1, |p_a|inf, |p_b|inf) (the fp64 subtract,
sum and square root); |angle - ref| <= ANGLE_CAP, the cap tests/test_device_geometry.py holds the device's relative pose
to (DEVICE["between"] on every quaternion component) through 2 atan2(|vec|, |w|): |d angle| <= 2 (|d vec| + |d w|) <=
2 (sqrt 3 + 1) cap for a unit quaternion, times max(1, |theta|) for SE2 headings.
Threshold ties (asserted on the reference, never on the device): no distance within 1e-9 search_radius of search_radius,
no angle within 1e-9 of max_angle, no two partners of one vertex closer in distance than 1e-9 search_radius, unless, in the
unjittered lattice alone, they are exactly equal by construction (spacing and offsets are powers of two: the border
distances are exactly search_radius and the id breaks the ties between equal distances).

The per-vertex cap: the issue asks the reference self-check "never more than 2m per vertex". That is not a property of
a symmetrised m-nearest-neighbour graph (a hub: five points around a centre, m = 1, the centre keeps five pairs;
test_reference_self_checks asserts this counter-example). What holds, and is asserted: a query's own picks are at most m,
every kept pair is somebody's pick, so at most m pairs per query are kept in all (the mean degree is at most 2m).

Stage B bounds (the issue's): beta = ||J||inf^2 1e-9 max|Sigma| + 1e-11 max|P_ref| of tests/test_relative_covariance.py for
sigma^2; |dz| <= |rho - range| beta / (2 sigma_ref^3) + dist bound / sigma_ref for zscore; the pass set equals the reference's
except pairs whose reference zscore is within that bound of z_max (at most 5 %; z_max is put into the widest gap of the
reference's zscores, so the reference leaves out none).
Measured on an MI355X, worst error over its bound: dist 0 (the device's distances equal numpy's bit for bit), SE3 angle
4.5e-2, SE2 angle 0; sigma^2 and zscore 4.0e-7 (intel NFR Tree), 1.7e-7 (sphere NFR Tree), 1.7e-5 (manhattan GLC Tree), 7.2e-8
(sphere GLC Tree), 5.8e-8 (sphere cliquey Subgraph); no pair within the zscore bound of z_max in any of the 20 runs. The
drifted loop: SE2 tight sigma 0.070 / zscore 3.59, loose 0.211 / 1.19; SE3 0.049 / 5.12 and 0.187 / 1.34.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from sparsifyposegraph_amd import abi, lib
from sparsifyposegraph_amd.lib import SpgError
from tests import oracle_lib, util
from tests import propose_ref as pr
from tests import relative_ref as rr
from tests.test_covariance_blocks import SMALL, _dense_blocks, _edge_pairs, _oracle_of, _small
from tests.test_device_geometry import DEVICE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")
_f64p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
EINVAL, ESTATE, ECAPACITY = -1, -7, -4
EPS = np.finfo(np.float64).eps
ANGLE_CAP = 2.0 * (np.sqrt(3.0) + 1.0) * DEVICE["between"]
TIE = 1e-9


# ------------------------------------------------------------------------------------------------- fixtures
def _orient(d, n, rng):
    if d == 3:
        return rng.uniform(-np.pi, np.pi, size=(n, 1))
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _graph(d, pos, seed, ids=None, chain=True):
    """graph dict: poses at `pos` with random orientations, ids a shuffled non-contiguous numbering unless given, and (chain)
    one edge between every two consecutive ids measured at the current relative pose"""
    rng = np.random.default_rng(seed)
    n = len(pos)
    poses = np.hstack([np.asarray(pos, np.float64), _orient(d, n, rng)])
    if ids is None:
        ids = 5 + 3 * rng.permutation(n)
    ids = np.asarray(ids, np.int32)
    order = np.argsort(ids)
    ij, data = [], []
    info = rr.upper(np.eye(d))
    if chain:
        for a, b in zip(order[:-1], order[1:]):
            ij.append((ids[a], ids[b]))
            data.append(np.concatenate([rr.between(d, poses[a], poses[b]), info]))
    return {"pose_dim": d, "ids": ids, "poses": poses, "edge_ij": np.array(ij, np.int32).reshape(-1, 2),
            "edge_data": np.array(data).reshape(len(ij), len(info) + (3 if d == 3 else 7))}


def _lattice(d, jitter_seed=None):
    """7 x 7 (SE2) / 4 x 4 x 4 (SE3) with spacing search_radius / 2 = 0.25, translated so that the coordinates straddle zero:
    every second pose sits on a cell border, some cells are negative. jitter_seed: a 1e-3 perturbation."""
    k = pr.dim(d)
    side = 7 if d == 3 else 4
    grid = np.array(np.meshgrid(*[np.arange(side)] * k, indexing="ij")).reshape(k, -1).T
    pos = (grid - side // 2) * 0.25
    if jitter_seed is not None:
        pos = pos + 1e-3 * np.random.default_rng(jitter_seed).uniform(-1, 1, size=pos.shape)
    return _graph(d, pos, seed=11 + d)


def _one_cell(d):
    """300 poses inside the cell [0, 0.5)^dim: more than a wavefront, more than 32 qualifying partners each"""
    pos = np.random.default_rng(300 + d).uniform(0.02, 0.48, size=(300, pr.dim(d)))
    return _graph(d, pos, seed=301 + d)


def _two_clusters(d, centre=5e5):
    """two clusters 10^6 apart on x (cell coordinates +-10^6 at radius 0.5), 40 poses each in a box of edge 1.2"""
    k = pr.dim(d)
    rng = np.random.default_rng(40 + d)
    pos = rng.uniform(-0.6, 0.6, size=(80, k))
    pos[:40, 0] -= centre
    pos[40:, 0] += centre
    pos[:, 1] -= 0.25 * centre
    return _graph(d, pos, seed=41 + d)


def _cloud(d, n, box, seed):
    return _graph(d, np.random.default_rng(seed).uniform(-box, box, size=(n, pr.dim(d))), seed=seed + 1)


# (name, builder, search_radius, list of keyword sets, exact ties allowed)
def _stage_a_cases(d):
    caps = [dict(max_per_vertex=m) for m in (0, 3)]
    return [
        ("lattice, unjittered", lambda: _lattice(d), 0.5, caps, True),
        ("lattice, jittered", lambda: _lattice(d, jitter_seed=2), 0.5,
         caps + [dict(max_angle=1.2), dict(min_id_gap=40), dict(max_angle=1.2, min_id_gap=40, max_per_vertex=2)], False),
        ("one cell", lambda: _one_cell(d), 0.5, [dict(max_per_vertex=m) for m in (1, 3, 32, 0)], False),
        ("two clusters", lambda: _two_clusters(d), 0.5, caps, False),
        ("cloud", lambda: _table_cloud(d), 0.3,
         [dict(), dict(max_per_vertex=4, max_angle=0.9, min_id_gap=30), dict(queries="last5"), dict(queries="last5", max_per_vertex=2)], False),
    ]


def _sorted_graph(g):
    o = np.argsort(g["ids"])
    return [int(i) for i in np.asarray(g["ids"])[o]], np.asarray(g["poses"])[o]


def _adjacent(pairs):
    return {(min(int(a), int(b)), max(int(a), int(b))) for a, b in pairs}


def _queries(ids, kw):
    kw = dict(kw)
    if kw.get("queries") == "last5":
        kw["queries"] = [int(i) for i in ids[-5:]]
    return kw


def _reference(d, ids, poses, adjacent, radius, kw):
    return pr.propose(d, ids, poses, adjacent, radius, kw.get("max_angle", 0.0), kw.get("min_id_gap", 1), kw.get("max_per_vertex", 0),
                      kw.get("queries"))


def _assert_no_ties(d, poses, ref, radius, max_angle, exact_ok, what):
    """the threshold-tie condition of the module docstring, on the reference alone"""
    dist = pr.distance_table(d, poses)
    near = np.abs(dist - radius) < TIE * radius
    if exact_ok:
        near &= dist != radius
    assert not near.any(), (what, "a distance within 1e-9 r of r")
    if max_angle > 0:
        n = len(poses)
        for a in range(n):
            for b in np.flatnonzero(dist[a] <= radius):
                if b > a:
                    assert abs(pr.rotation_angle(d, poses[a], poses[int(b)]) - max_angle) >= TIE, (what, "an angle within 1e-9 of max_angle")
    for v, lst in ref["partners"].items():
        ds = np.array([x[0] for x in lst])
        gaps = np.diff(ds)
        bad = gaps < TIE * radius
        if exact_ok:
            bad &= gaps != 0
        assert not bad.any(), (what, "two partners of one vertex within 1e-9 r", v)


# ------------------------------------------------------------------------------------------------------- CPU
def test_reference_self_checks():
    """The kept set equals the union of the per-vertex picks computed by sorting every row of the distance table; every
    query's own picks are at most m and at most m pairs per query are kept; m = 0 keeps every qualifying pair; a hub keeps
    more than 2m pairs (module docstring); cells_tested equals a brute-force count over integer cell differences."""
    for d in (3, 6):
        g = _cloud(d, 250, 1.0, 5 + d)
        ids, poses = _sorted_graph(g)
        adjacent = _adjacent(g["edge_ij"])
        radius = 0.45
        full = pr.propose(d, ids, poses, adjacent, radius, m=0)
        assert len(full["ij"]) == full["n_qualifying"] == len(full["qualifying"]) > 400
        dist = pr.distance_table(d, poses)
        for m in (1, 3, 8):
            ref = pr.propose(d, ids, poses, adjacent, radius, m=m)
            picks = set()
            for a in range(len(ids)):
                cand = [(dist[a, b], ids[b], b) for b in range(len(ids))
                        if b != a and dist[a, b] <= radius and (min(ids[a], ids[b]), max(ids[a], ids[b])) not in adjacent]
                mine = sorted(cand)[:m]
                assert len(mine) <= m
                picks.update((min(ids[a], ids[b]), max(ids[a], ids[b])) for _, _, b in mine)
            assert {tuple(p) for p in ref["ij"].tolist()} == picks                       # symmetric: a picks b or b picks a
            assert len(ref["ij"]) <= m * len(ids) and len(ref["ij"]) <= len(full["ij"])
            assert [tuple(p) for p in ref["ij"].tolist()] == sorted(picks)              # ascending (id_a, id_b), every pair once
        # a query list: only pairs with a query endpoint, each query at most m picks
        q = ids[-5:]
        ref = pr.propose(d, ids, poses, adjacent, radius, m=2, queries=q)
        assert len(ref["ij"]) <= 2 * 5 and all(a in q or b in q for a, b in ref["ij"].tolist())
        p = poses[:, :pr.dim(d)]
        cell = np.floor(p / radius).astype(np.int64)
        brute = int((np.abs(cell[:, None, :] - cell[None, :, :]).max(axis=2) <= 1).sum()) - len(ids)
        assert pr.cells_tested(p, radius) == brute
        mask = np.isin(ids, q)
        assert pr.cells_tested(p, radius, mask) == int((np.abs(cell[mask][:, None, :] - cell[None, :, :]).max(axis=2) <= 1).sum()) - 5
    # the hub: the centre keeps five pairs at m = 1
    ang = 2 * np.pi * np.arange(5) / 5
    pos = np.vstack([[0.0, 0.0], np.c_[np.cos(ang), np.sin(ang)] * (1 + 0.01 * np.arange(5))[:, None]])
    hub = _graph(3, pos, seed=3, ids=np.arange(6), chain=False)
    ref = pr.propose(3, *_sorted_graph(hub), set(), 1.1, m=1)
    assert ref["ij"].tolist() == [[0, b] for b in range(1, 6)]


@pytest.mark.parametrize("d", [3, 6])
def test_fixtures_have_no_threshold_ties(d):
    """Every stage-A fixture of the GPU tests satisfies the tie condition of the module docstring (the jitter seeds were chosen
    for it); the unjittered lattice has pairs at exactly search_radius and equal partner distances, and keeps them."""
    for name, build, radius, kws, exact_ok in _stage_a_cases(d):
        g = build()
        ids, poses = _sorted_graph(g)
        for kw in kws:
            kw = _queries(ids, kw)
            ref = _reference(d, ids, poses, _adjacent(g["edge_ij"]), radius, kw)
            _assert_no_ties(d, poses, ref, radius, kw.get("max_angle", 0.0), exact_ok, (name, d, kw))
            assert len(ref["ij"]) > 0
        if exact_ok:
            ref = _reference(d, ids, poses, _adjacent(g["edge_ij"]), radius, {})
            assert (ref["dist"] == radius).sum() > 20 and any(np.any(np.diff([x[0] for x in l]) == 0) for l in ref["partners"].values())


def test_abi_and_bindings_cover_the_proposal():
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    L = C.CDLL(lib.LIB_PATH)
    assert "spg_graph_propose_candidates" in lib.SYMBOLS and hasattr(L, "spg_graph_propose_candidates")
    assert C.sizeof(abi.ProposeStats) == C.sizeof(abi.CovSolveStats) + 56
    assert set(abi.ProposeStats().asdict()) == {"n_cells", "max_cell_population", "table_slots", "pairs_tested", "n_qualifying", "n_kept", "n_gated",
                                                "device_seconds", "solve"}
    assert callable(GraphWrapperHIP.proposeCandidates)
    hdr = open(os.path.join(ROOT, "include", "spg.h")).read()
    assert "spg_propose_stats" in hdr and "SPG_PROPOSE_TABLE_BITS" in hdr and "AFTER the cap" in hdr
    assert "proposeCandidates" in open(os.path.join(ROOT, "include", "spg_graph_wrapper.hpp")).read()
    stubs = open(os.path.join(ROOT, "tools", "asan_stubs.cpp")).read()
    assert "hip_propose_search" in stubs and "hip_propose_gate" in stubs


def test_proposal_checks_arguments_before_the_backend():
    """On an injected (CPU) context: search_radius <= 0 / inf / NaN, max_per_vertex outside 0 .. 32, range above search_radius,
    z_max = NaN, an unknown and a repeated query id, an unknown fixed vertex and an active stepwise marginalisation are
    SPG_EINVAL with the offending value or id in the text; one live vertex and an empty query list return 0; a call that
    would compute is SPG_ESTATE (no CPU fallback); the Python layer raises."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    sub = _small()
    ictx = oracle_lib.injected_context()
    a = GraphWrapperHIP.from_dict(sub, ctx=ictx)
    L = a.L
    ids = np.ascontiguousarray(sub["ids"][:5], np.int32)
    err = lambda: L.spg_last_error(ictx.h).decode()  # noqa: E731
    st = abi.ProposeStats()

    def call(radius=1.0, max_angle=0.0, gap=1, m=0, q=None, rng=0.0, z_max=2.0, fid=-1, h=a.h):
        qp = None if q is None else np.ascontiguousarray(q, np.int32)
        return L.spg_graph_propose_candidates(h, fid, radius, max_angle, gap, m, None if qp is None else qp.ctypes.data_as(_i32p), 0 if qp is None else len(qp),
                                              rng, z_max, None, None, None, None, None, 0, C.byref(st))
    assert call() == ESTATE and "HIP backend" in err() and "spg_graph_propose_candidates" in err()
    assert call(q=ids, rng=0.5, m=3) == ESTATE
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert call(radius=bad) == EINVAL and "search_radius" in err()
    for bad in (-1, 33):
        assert call(m=bad) == EINVAL and "max_per_vertex" in err() and str(bad) in err()
    assert call(radius=1.0, rng=1.5) == EINVAL and "range" in err() and "1.5" in err()
    assert call(rng=np.nan) == EINVAL and "range" in err()
    assert call(z_max=np.nan) == EINVAL and "z_max" in err()
    assert call(max_angle=np.nan) == EINVAL and "max_angle" in err()
    assert call(q=[int(ids[0]), 999999]) == EINVAL and "999999" in err() and "query 1" in err()
    assert call(q=[int(ids[0]), int(ids[1]), int(ids[0])]) == EINVAL and "twice" in err() and str(int(ids[0])) in err() and "query 2" in err()
    assert call(fid=999999) == EINVAL and "fixed vertex" in err() and "999999" in err()
    assert call(q=np.zeros(0, np.int32)) == 0                       # an empty query list
    assert L.spg_graph_propose_candidates(None, -1, 1.0, 0.0, 1, 0, None, 0, 0.0, 2.0, None, None, None, None, None, 0, None) == EINVAL
    one = GraphWrapperHIP(ctx=ictx, pose_dim=3)
    assert call(h=one.h) == 0                                        # no vertex
    one.addVertex(7, [0.0, 0.0, 0.0])
    assert call(h=one.h) == 0 and st.n_kept == 0                     # one live vertex
    g, which, opts, *_ = util.load_golden("intel_nfr_tree_sp3")
    sub2, w = util.prefix_graph(g, which, 30)
    b = GraphWrapperHIP.from_dict(sub2, ctx=ictx)
    b.begin(w, opts, 0, 1)
    assert call(h=b.h) == EINVAL and "active" in err()
    with pytest.raises(SpgError, match="HIP backend"):
        a.proposeCandidates(1.0)
    with pytest.raises(SpgError, match="search_radius"):
        a.proposeCandidates(0.0)
    with pytest.raises(SpgError, match="range"):
        a.proposeCandidates(1.0, range=2.0)
    with pytest.raises(SpgError, match="999999"):
        a.proposeCandidates(1.0, queries=[999999])
    with pytest.raises(SpgError, match="max_per_vertex"):
        a.proposeCandidates(1.0, max_per_vertex=33)
    got = one.proposeCandidates(1.0, stats=True)
    assert got["ij"].shape == (0, 2) and got["dist"].shape == (0,) and got["angle"].shape == (0,) and got["stats"]["n_kept"] == 0


def _build_demo(tmp_path):
    exe = str(tmp_path / "propose_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "propose_demo.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_propose_demo_compiles(tmp_path):
    out = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr


# ------------------------------------------------------------------------------------------------------- GPU
def _check_stage_a(hg, d, radius, kw, exact_ok, what, adjacent=None):
    """one device run (twice) against the reference; returns (got, ref)"""
    ids, poses = hg.vertices()
    o = np.argsort(ids)
    ids, poses = [int(i) for i in ids[o]], poses[o]
    if adjacent is None:
        adjacent = _adjacent(_edge_pairs(hg))
    kw = _queries(ids, kw)
    ref = _reference(d, ids, poses, adjacent, radius, kw)
    _assert_no_ties(d, poses, ref, radius, kw.get("max_angle", 0.0), exact_ok, what)
    got = hg.proposeCandidates(radius, stats=True, **kw)
    again = hg.proposeCandidates(radius, stats=True, **kw)
    assert got["ij"].dtype == np.int32 and np.array_equal(got["ij"], ref["ij"]), (what, len(got["ij"]), len(ref["ij"]))
    for key in ("ij", "dist", "angle"):
        assert got[key].tobytes() == again[key].tobytes(), (what, key)
    s = got["stats"]
    k = pr.dim(d)
    qmask = None if kw.get("queries") is None else np.isin(ids, kw["queries"])
    assert s["pairs_tested"] == pr.cells_tested(poses[:, :k], radius, qmask), what
    assert s["n_qualifying"] == ref["n_qualifying"] and s["n_kept"] == s["n_gated"] == len(ref["ij"]), what
    cells = {tuple(c) for c in np.floor(poses[:, :k] / radius).astype(np.int64)}
    assert s["n_cells"] == len(cells) and s["table_slots"] >= 2 * len(ids) and s["table_slots"] & (s["table_slots"] - 1) == 0
    assert s["device_seconds"] > 0 and s["solve"]["columns"] == 0
    at = {v: i for i, v in enumerate(ids)}
    worst_d = worst_a = 0.0
    for (a, b), dd, aa, rd, ra in zip(got["ij"].tolist(), got["dist"], got["angle"], ref["dist"], ref["angle"]):
        pa, pb = poses[at[a]], poses[at[b]]
        bound = 16 * EPS * max(1.0, np.abs(pa[:k]).max(), np.abs(pb[:k]).max())
        worst_d = max(worst_d, abs(dd - rd) / bound)
        cap = ANGLE_CAP * (max(1.0, abs(pa[2]), abs(pb[2])) if d == 3 else 1.0)
        worst_a = max(worst_a, abs(aa - ra) / cap)
    print(f"{what}: {len(ref['ij'])} pairs of {ref['n_qualifying']} qualifying, {s['pairs_tested']} tests, worst dist error / bound {worst_d:.2e}, "
          f"angle error / cap {worst_a:.2e}")
    assert worst_d <= 1.0 and worst_a <= 1.0, (what, worst_d, worst_a)
    return got, ref


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_stage_a_equals_the_reference(d, hip_ctx):
    """(a) the lattices on cell borders, unjittered bit for bit; (b) 300 poses in one cell at m = 1, 3, 32, 0; (c) two clusters
    10^6 apart; (f) the last five ids as queries; (h) max_angle and min_id_gap on and off; on each: ij exactly, two calls
    bit-identical, pairs_tested = the grid's count, dist and angle within their bounds."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    for name, build, radius, kws, exact_ok in _stage_a_cases(d):
        g = build()
        hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
        adjacent = _adjacent(g["edge_ij"])
        for kw in kws:
            got, ref = _check_stage_a(hg, d, radius, kw, exact_ok, f"SE{2 if d == 3 else 3} {name} {kw}", adjacent)
            if name == "one cell":
                assert got["stats"]["max_cell_population"] == 300 and got["stats"]["n_cells"] == 1
                assert min(len(l) for l in ref["partners"].values()) > 32
            if exact_ok and not kw.get("max_per_vertex"):
                assert (got["dist"] == radius).sum() == (ref["dist"] == radius).sum() > 20      # the <= at exactly search_radius
        if name == "two clusters":
            assert np.abs(np.floor(g["poses"][:, 0] / radius)).min() > 9e5          # cell coordinates near the 21-bit limit


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_small_graphs_empty_results_and_poses_outside_the_grid(d, hip_ctx):
    """(d) n = 1, n = 2 (a pair, and no pair when an edge joins the two) and a radius that yields nothing; a pose whose cell
    coordinate does not fit 21 bits is SPG_ECAPACITY with its id, one that is not finite SPG_EINVAL with its id."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    k = pr.dim(d)
    one = GraphWrapperHIP.from_dict(_graph(d, np.zeros((1, k)), seed=1), ctx=hip_ctx)
    assert len(one.proposeCandidates(1.0)["ij"]) == 0
    pos = np.zeros((2, k))
    pos[1, 0] = 0.3
    two = GraphWrapperHIP.from_dict(_graph(d, pos, seed=2, ids=[4, 9], chain=False), ctx=hip_ctx)
    got = two.proposeCandidates(1.0, stats=True)
    assert got["ij"].tolist() == [[4, 9]] and got["dist"][0] == 0.3 and got["stats"]["pairs_tested"] == 2
    assert len(two.proposeCandidates(0.2)["ij"]) == 0 and len(two.proposeCandidates(1.0, min_id_gap=6)["ij"]) == 0
    assert two.proposeCandidates(1.0, min_id_gap=5)["ij"].tolist() == [[4, 9]]
    joined = GraphWrapperHIP.from_dict(_graph(d, pos, seed=2, ids=[4, 9], chain=True), ctx=hip_ctx)
    assert len(joined.proposeCandidates(1.0)["ij"]) == 0
    cloud = GraphWrapperHIP.from_dict(_cloud(d, 200, 1.0, 9), ctx=hip_ctx)
    got = cloud.proposeCandidates(1e-4, stats=True)
    assert len(got["ij"]) == 0 and got["stats"]["n_kept"] == 0
    far = _two_clusters(d, centre=6e5)
    hg = GraphWrapperHIP.from_dict(far, ctx=hip_ctx)
    with pytest.raises(SpgError, match="21 bits") as e:
        hg.proposeCandidates(0.5)
    ids, poses = _sorted_graph(far)
    first = next(i for i, p in zip(ids, poses) if not -2 ** 20 <= np.floor(p[0] / 0.5) < 2 ** 20)
    assert f"vertex {first} " in str(e.value) and f"code {ECAPACITY}" in str(e.value)
    assert len(hg.proposeCandidates(1.0)["ij"]) > 0                                      # the same poses fit at radius 1
    for bad in (np.nan, np.inf):                                                         # a pose that is not finite: SPG_EINVAL with its id
        pos3 = np.zeros((3, k))
        pos3[:, 0] = [0.0, 0.3, 0.6]
        g3 = _graph(d, pos3, seed=3, ids=[4, 8, 9], chain=False)
        g3["poses"][1, k - 1] = bad
        with pytest.raises(SpgError, match="not finite") as e:
            GraphWrapperHIP.from_dict(g3, ctx=hip_ctx).proposeCandidates(1.0)
        assert "vertex 8 " in str(e.value) and f"code {EINVAL}" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["intel_nfr_tree_sp3", "sphere_glc_tree"])
def test_marginalised_graphs(case, hip_ctx):
    """(e) every second vertex marginalised: the ids are non-contiguous and the edges the removal created (n-ary under GLC)
    take part in rule 4; the pairs go unchanged into relativeCovariances, scoreCandidates and compatibleCandidates."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, which, opts, *_ = util.load_golden(case)
    sub, _ = util.prefix_graph(g, which, 80)
    d = sub["pose_dim"]
    hg = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx, useGLC=opts.algorithm == abi.ALG_GLC)
    w = np.asarray(sub["ids"], np.int32)[1:-1:2]
    st = hg.marginalizeNoOptimize(w, opts)
    assert st["n_bad_status"] == 0 and st["n_removed"] == len(w)
    ids, poses = hg.vertices()
    dist = pr.distance_table(d, poses)
    radius = float(np.sort(dist, axis=1)[:, 6].mean()) * 1.0000001
    edges = _adjacent(_edge_pairs(hg))
    got, ref = _check_stage_a(hg, d, radius, dict(max_per_vertex=3), False, f"{case} marginalised")
    assert len(got["ij"]) > 10 and not ({tuple(p) for p in got["ij"].tolist()} & edges)
    near = {(min(int(ids[a]), int(ids[b])), max(int(ids[a]), int(ids[b]))) for a, b in zip(*np.nonzero(dist <= radius)) if a != b}
    assert near & edges                                                                  # rule 4 had something to exclude
    if opts.algorithm == abi.ALG_GLC:
        assert set(int(x) for x in hg.edges()["kind"]) != {abi.EDGE_BINARY}
    # plumbing: the first pair is accepted unchanged by the later stages
    first = got["ij"][:1]
    rel, P = hg.relativeCovariances(first)
    info = rr.upper(np.linalg.inv(P[0] + 1e-3 * np.eye(d)))
    assert hg.scoreCandidates(first, rel, [info])["status"][0] == abi.CAND_SCORED
    assert hg.compatibleCandidates(first, rel, [info], joint_max_d2=False)["compatible"].tolist() == [0]


TABLE_CHILD = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
os.environ["SPG_PROPOSE_TABLE_BITS"] = sys.argv[2]
import numpy as np
from sparsifyposegraph_amd.lib import Context, SpgError
from sparsifyposegraph_amd.graph import GraphWrapperHIP
from tests import test_candidate_proposal as t
d = int(sys.argv[4])
hg = GraphWrapperHIP.from_dict(t._table_cloud(d), ctx=Context(0))
try:
    got = hg.proposeCandidates(0.3, max_per_vertex=4, stats=True)
    np.savez(os.path.join(sys.argv[3], "table.npz"), ij=got["ij"], dist=got["dist"], angle=got["angle"], slots=got["stats"]["table_slots"])
    print("ran", got["stats"]["table_slots"])
except SpgError as e:
    print("refused", e)
'''


def _table_cloud(d):
    return _cloud(d, 700, 2.0 if d == 3 else 1.2, 70 + d)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_forced_small_table_gives_the_same_pairs(d, tmp_path, hip_ctx):
    """(g) SPG_PROPOSE_TABLE_BITS at the smallest admissible value (a table more than half full: long probe chains, lookups
    of absent cells that walk them) in a fresh process returns the bits of the default table; one bit less is SPG_ECAPACITY."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    hg = GraphWrapperHIP.from_dict(_table_cloud(d), ctx=hip_ctx)
    want = hg.proposeCandidates(0.3, max_per_vertex=4, stats=True)
    cells = want["stats"]["n_cells"]
    bits = int(np.ceil(np.log2(cells)))
    assert 2 ** (bits - 1) < cells <= 2 ** bits < want["stats"]["table_slots"] and len(want["ij"]) > 500
    script = tmp_path / "table_child.py"
    script.write_text(TABLE_CHILD)
    out = subprocess.run([sys.executable, str(script), ROOT, str(bits), str(tmp_path), str(d)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ran" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    got = np.load(str(tmp_path / "table.npz"))
    assert int(got["slots"]) == 2 ** bits
    for key in ("ij", "dist", "angle"):
        assert got[key].tobytes() == want[key].tobytes(), key
    out = subprocess.run([sys.executable, str(script), ROOT, str(bits - 1), str(tmp_path), str(d)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "refused" in out.stdout and "occupied cells" in out.stdout and f"code {ECAPACITY}" in out.stdout, \
        out.stdout[-2000:] + out.stderr[-3000:]


# ------------------------------------------------------------------------------------------------------- stage B
def _gate_reference(d, poses_of, blk, scale, ij, rng):
    """per pair: rho, sigma, zscore of the reference, beta and the zscore bound"""
    k = pr.dim(d)
    out = []
    for a, b in ij.tolist():
        S = np.block([[blk(a, a), blk(a, b)], [blk(b, a), blk(b, b)]])
        rho, sg, z, J, P = pr.gate(d, poses_of[a], poses_of[b], S, rng)
        beta = np.abs(J).sum(axis=1).max() ** 2 * 1e-9 * scale + 1e-11 * np.abs(P).max()
        dbound = 16 * EPS * max(1.0, np.abs(poses_of[a][:k]).max(), np.abs(poses_of[b][:k]).max())
        zb = abs(rho - rng) * beta / (2 * sg ** 3) + dbound / sg
        out.append((rho, sg, z, beta, zb))
    return np.array(out).reshape(-1, 5)


def _widest_gap(z):
    """z_max in the widest gap between consecutive positive reference zscores (pairs beyond range, where z_max decides), taken
    in their middle half: the reference decides every pair"""
    s = np.sort(z[np.isfinite(z) & (z > 0)])
    lo, hi = len(s) // 4, max(3 * len(s) // 4, len(s) // 4 + 2)
    g = np.diff(s[lo:hi])
    i = int(np.argmax(g))
    return 0.5 * (s[lo + i] + s[lo + i + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", SMALL)
def test_range_gate_equals_the_dense_inverse_on_small_graphs(case, n, hip_ctx):
    """The small graphs of the covariance tests before and after their marginalisation, both gauges, 40 spread queries (the
    fixed vertex among them), m = 4, range = 0.6 search_radius: sigma^2 within beta of u^T P_ref u, zscore within its bound, the
    pass set equal to the reference's (z_max in the widest gap of the reference's zscores; at most 5 % may be left out as
    within the bound of z_max, and the reference leaves out none); z_max = -10 keeps exactly the pairs with rho <= range;
    stage A's pairs are unchanged by the gate."""
    from tests.test_relative_covariance import _small_graphs
    sub, graphs, kept = _small_graphs(case, n, hip_ctx)
    d = sub["pose_dim"]
    worst_s = worst_z = 0.0
    with_fixed = 0
    for hg, og in graphs:
        ids, poses = hg.vertices()
        o = np.argsort(ids)
        ids, poses = [int(i) for i in ids[o]], poses[o]
        poses_of = dict(zip(ids, poses))
        dist = pr.distance_table(d, poses)
        radius = float(np.sort(dist, axis=1)[:, 8].mean())
        rng_ = 0.6 * radius
        for fid in (ids[0], kept[len(kept) // 2]):
            queries = sorted(set(ids[::max(len(ids) // 40, 1)]) | {fid})
            kw = dict(max_per_vertex=4, min_id_gap=3, queries=queries)
            Sig = np.linalg.inv(og.information(fid))
            blk = _dense_blocks(Sig, ids, fid, d)
            stage_a = hg.proposeCandidates(radius, **kw)
            everything = hg.proposeCandidates(radius, range=rng_, z_max=1e300, fixed_id=fid, stats=True, **kw)
            assert np.array_equal(everything["ij"], stage_a["ij"]) and len(stage_a["ij"]) > 30
            with_fixed += sum(fid in p for p in stage_a["ij"].tolist())
            s = everything["stats"]
            assert s["n_gated"] == s["n_kept"] == len(stage_a["ij"]) and 0 < s["solve"]["columns"] <= len(ids) and s["solve"]["solve_seconds"] > 0
            ref = _gate_reference(d, poses_of, blk, float(np.abs(Sig).max()), everything["ij"], rng_)
            rho, sg, z, beta, zb = ref.T
            assert np.all(sg > 0)
            es = np.abs(everything["sigma"] ** 2 - sg ** 2) / beta
            ez = np.abs(everything["zscore"] - z) / zb
            worst_s, worst_z = max(worst_s, es.max()), max(worst_z, ez.max())
            assert es.max() <= 1.0 and ez.max() <= 1.0, (case, fid, es.max(), ez.max())
            z_max = _widest_gap(z)
            unsure = np.abs(z - z_max) <= zb
            assert not unsure.any() and unsure.sum() <= 0.05 * len(z)
            want = (z <= z_max) | (rho <= rng_)
            assert 0 < want.sum() < len(want), (case, fid, "the gate decides nothing")
            gated = hg.proposeCandidates(radius, range=rng_, z_max=z_max, fixed_id=fid, stats=True, **kw)
            assert np.array_equal(gated["ij"], everything["ij"][want]) and gated["stats"]["n_gated"] == int(want.sum())
            assert np.array_equal(gated["zscore"], everything["zscore"][want]) and np.array_equal(gated["sigma"], everything["sigma"][want])
            inside = hg.proposeCandidates(radius, range=rng_, z_max=-10.0, fixed_id=fid, **kw)
            keep = (rho <= rng_) | (z <= -10.0)
            assert np.abs(rho - rng_).min() > 1e-9 * radius
            assert np.array_equal(inside["ij"], everything["ij"][keep]) and np.all(inside["zscore"] <= 0) and (rho <= rng_).sum() > 0
    assert with_fixed > 0                                            # the fixed vertex was an endpoint of some pair
    print(f"{case}[{n}]: worst sigma^2 error / beta {worst_s:.2e}, worst zscore error / bound {worst_z:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_tight_and_loose_pairs_beyond_range_get_opposite_verdicts(d, hip_ctx):
    """The drifted loop of tests/test_candidate_compatibility.py: a pair two odometry steps apart (tight) and a pair across
    the loop (loose), each asked with range = its own estimated distance - 0.25, z_max = 2: the tight pair is dropped, the loose
    one stays, as the reference on the oracle's dense covariance says."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    from tests.test_candidate_compatibility import _chain
    g, _ = _chain(d)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    ids, poses = _sorted_graph(g)
    fid = 0
    Sig = np.linalg.inv(oracle_lib.OracleGraph.from_dict(g).information(fid))
    blk = _dense_blocks(Sig, ids, fid, d)
    dist = pr.distance_table(d, poses)
    tight = (10, 12)
    loose = min(((a, b) for a in range(3, 9) for b in range(29, 35)), key=lambda p: abs(dist[p] - dist[tight]))
    verdict = {}
    for name, (a, b) in (("tight", tight), ("loose", loose)):
        S = np.block([[blk(a, a), blk(a, b)], [blk(b, a), blk(b, b)]])
        rng_ = float(dist[a, b]) - 0.25
        rho, sg, z, *_ = pr.gate(d, poses[a], poses[b], S, rng_)
        radius = float(dist[a, b]) * 1.01
        got = hg.proposeCandidates(radius, min_id_gap=2, queries=[a], range=rng_, z_max=2.0, fixed_id=fid)
        everything = hg.proposeCandidates(radius, min_id_gap=2, queries=[a], range=rng_, z_max=1e300, fixed_id=fid)
        row = everything["ij"].tolist().index([a, b])
        assert everything["zscore"][row] == pytest.approx(z, rel=1e-6) and everything["sigma"][row] == pytest.approx(sg, rel=1e-6)
        verdict[name] = ([a, b] in got["ij"].tolist(), z, sg)
        print(f"SE{2 if d == 3 else 3} {name} pair {(a, b)}: rho {rho:.3f}, sigma {sg:.3f}, zscore {z:.2f}, kept {verdict[name][0]}")
    assert verdict["tight"][1] > 2.0 > verdict["loose"][1] and verdict["tight"][2] < verdict["loose"][2]
    assert verdict["tight"][0] is False and verdict["loose"][0] is True
