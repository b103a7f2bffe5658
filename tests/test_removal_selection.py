"""The vertices to remove, chosen on the device by spatial redundancy (spg_graph_select_removals, csrc/spg_removals.inc)
against the plain numpy rule of tests/removals_ref.py.
CPU: the reference against itself on every fixture of the GPU tests (the sequential rule and the synchronous rounds give the
same kept set; every removed vertex has a kept vertex within radius; unforced kept vertices are pairwise not redundant; a
second pass over the kept set removes nothing), the fixtures free of angle ties, the argument contract on an injected
backend, the ABI and the bindings, the C++ demo compiles.
GPU, SE2 and SE3, n <= 700: the fixtures of tests/test_candidate_proposal.py (the unjittered lattice with exact ties at the
radius, poses on cell borders and negative cells; the jittered one with max_angle; 300 poses in one cell; two clusters 10^6
apart; the cloud of the table test), each in hash order, "oldest", "newest" and a random priority with repeated values, each
with no, five and two mutually redundant forced vertices; a chain of 256 dependent decisions; a forced small cell table in a
child process; n = 0 / 1 / 2, everything forced, radii below and above every distance, poses outside the grid; marginalised
golden graphs; selection, marginalisation and a second selection end to end.

What the equality tests assert: removed and representative equal the reference's, rep_dist bit for bit (pp_dist rounds every
product and sum on its own, as numpy does: tests/test_candidate_proposal.py measured 0 difference), two calls return the same
bytes, the counters add up. Ties: an exact distance tie at the radius or between two representatives is decided by the same
<= and the same (dist, id) order on both sides, so it is allowed; with max_angle > 0 no pair within radius may have its angle
within 1e-9 of max_angle (asserted on the reference, never on the device).
The one-cell fixture is asked at radius 0.8: its poses lie in [0.02, 0.48]^dim, at most 0.46 sqrt(3) < 0.8 apart, so every
pair is redundant, one cell [0, 0.8)^dim holds all 300, and exactly one unforced vertex is kept (none when a vertex is forced).
Rounds: the device decides in launch k at least what the synchronous rounds of the reference decide in round k (a verdict
needs only verdicts of earlier rounds, which earlier launches have written), so rounds <= depth; the tests allow depth + 1.
Measured on an MI355X: all 120 fixture runs equal, rep_dist bit for bit; the line of 256 in "oldest" order 169 (SE2) and 170
(SE3) rounds for a depth of 171, in hash order 6 for a depth of 6; the 700-pose cloud 6 to 9 rounds in every order; end to
end 362 of 600 removed, KLD 18.8.
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
from tests import removals_ref as rf
from tests.test_candidate_proposal import (_cloud, _graph, _lattice, _one_cell, _sorted_graph, _table_cloud, _two_clusters)
from tests.test_covariance_blocks import SMALL, _small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")
_f64p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
EINVAL, ESTATE, ECAPACITY = -1, -7, -4
TIE = 1e-9
ORDERS = ("hash", "oldest", "newest", "random")
KEEPS = ("none", "five", "pair")


# ------------------------------------------------------------------------------------------------- fixtures
# (name, builder, radius, max_angle)
def _cases(d):
    return [("lattice, unjittered", lambda: _lattice(d), 0.5, 0.0),
            ("lattice, jittered", lambda: _lattice(d, jitter_seed=2), 0.5, 1.2),
            ("one cell", lambda: _one_cell(d), 0.8, 0.0),
            ("two clusters", lambda: _two_clusters(d), 0.5, 0.0),
            ("cloud", lambda: _table_cloud(d), 0.3, 0.0)]


@functools.lru_cache(maxsize=None)
def _case(d, name):
    """the fixture once per session: graph dict, sorted ids and poses, radius, max_angle, the redundancy table (read only)"""
    _, build, radius, max_angle = next(c for c in _cases(d) if c[0] == name)
    g = build()
    ids, poses = _sorted_graph(g)
    red, dist = rf.redundancy(d, poses, radius, max_angle)
    red.setflags(write=False); dist.setflags(write=False)
    return g, ids, poses, radius, max_angle, (red, dist)


def _priority(ids, order, seed=5):
    """hash: None; "oldest" / "newest"; random: an array of eight distinct values, so that most ties go to the id"""
    if order == "hash":
        return None
    if order == "random":
        return np.random.default_rng(seed).integers(0, 8, size=len(ids)).astype(np.float64)
    return order


def _keep(ids, red, which):
    if which == "none":
        return []
    if which == "five":
        return [int(ids[i]) for i in np.linspace(0, len(ids) - 1, 5).astype(int)][::-1]      # not in id order
    a, b = np.argwhere(np.triu(red))[len(ids) // 3]
    return [int(ids[b]), int(ids[a])]


def _check_properties(ref, ids, radius, what):
    """the three consequences of the rule, on a reference result"""
    kept, red, dist = ref["kept"], ref["red"], ref["dist"]
    forced = np.zeros(len(ids), bool)
    forced[ref["order"][:ref["n_forced"]]] = True
    assert kept[forced].all(), what
    for v in np.flatnonzero(~kept):
        assert (dist[v][kept] <= radius).any(), (what, "a removed vertex without a kept vertex within radius", ids[v])
    free = np.flatnonzero(kept & ~forced)
    assert not red[np.ix_(free, free)].any(), (what, "two unforced kept vertices are redundant")
    assert len(ref["removed"]) == (~kept).sum() and np.all(np.diff(ref["removed"]) > 0)
    at = {v: i for i, v in enumerate(ids)}
    for v, r, dd in zip(ref["removed"], ref["representative"], ref["rep_dist"]):
        assert kept[at[int(r)]] and red[at[int(v)], at[int(r)]] and dd == dist[at[int(v)], at[int(r)]] <= radius


# ------------------------------------------------------------------------------------------------------- CPU
def test_mix64_is_the_splitmix64_finaliser():
    """Known values of the finaliser (computed with Python integers), and what the order hashes: the id as uint32."""
    def py(x):
        m = (1 << 64) - 1
        x ^= x >> 30; x = x * 0xbf58476d1ce4e5b9 & m
        x ^= x >> 27; x = x * 0x94d049bb133111eb & m
        return x ^ (x >> 31)
    xs = [0, 1, 2, 12345, 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 63 + 7]
    assert [int(v) for v in rf.mix64(np.array(xs, np.uint64))] == [py(x) for x in xs]
    assert py(0) == 0 and py(0x9e3779b97f4a7c15) == 0xe220a8397b1dcdaf               # SplitMix64's first output from seed 0
    order, nf = rf.order_of([3, 5, 9, 11], keep=[9])
    assert nf == 0 + 1 and order[0] == 2 and sorted(order) == [0, 1, 2, 3]
    assert [[3, 5, 9, 11][i] for i in order[1:]] == sorted([3, 5, 11], key=py)
    assert rf.order_of([3, 5, 9], priority="oldest")[0] == [0, 1, 2] and rf.order_of([3, 5, 9], priority="newest")[0] == [2, 1, 0]
    assert rf.order_of([3, 5, 9], priority=[1.0, 2.0, 2.0])[0] == [1, 2, 0]                  # descending, the tie to the id
    assert rf.order_of([3, 5, 9], priority={3: 0.0, 5: -0.0, 9: -1.0})[0] == [0, 1, 2]       # -0.0 equals 0.0


@pytest.mark.parametrize("d", [3, 6])
def test_reference_self_checks(d):
    """On every fixture, order and keep list of the GPU tests: the sequential rule and the synchronous rounds give the same
    kept set; every removed vertex has a kept vertex within radius; unforced kept vertices are pairwise not redundant; the
    representative is kept, redundant and at the reported distance; a second pass over the kept set removes nothing."""
    for name, *_ in _cases(d):
        g, ids, poses, radius, max_angle, table = _case(d, name)
        for order in ORDERS:
            for which in KEEPS:
                what = (name, d, order, which)
                keep = _keep(ids, table[0], which)
                prio = _priority(ids, order)
                ref = rf.select(d, ids, poses, radius, max_angle, keep, prio, table=table)
                kept2, depth = rf.rounds(table[0], ref["order"], ref["n_forced"])
                assert np.array_equal(ref["kept"], kept2) and 0 < depth <= len(ids), what
                _check_properties(ref, ids, radius, what)
                assert 0 < len(ref["removed"]) < len(ids), what
                k = np.flatnonzero(ref["kept"])
                vals = rf.priority_values(ids, prio)
                again = rf.select(d, [ids[i] for i in k], poses[k], radius, max_angle, keep, None if vals is None else vals[k])
                assert len(again["removed"]) == 0, what
        if name == "one cell":
            assert table[0].sum() == 300 * 299 and len({tuple(c) for c in np.floor(poses[:, :pr.dim(d)] / radius)}) == 1
        if name == "lattice, unjittered":
            assert (table[1] == radius).sum() > 20                                       # exact ties at the radius


@pytest.mark.parametrize("d", [3, 6])
def test_fixtures_have_no_angle_ties(d):
    """With max_angle > 0 no pair within radius has its angle within 1e-9 of max_angle; the angle rule decides something."""
    for name, *_ in _cases(d):
        g, ids, poses, radius, max_angle, (red, dist) = _case(d, name)
        if not max_angle > 0:
            continue
        dropped = 0
        for a, b in zip(*np.nonzero(np.triu(dist <= radius, 1))):
            ang = pr.rotation_angle(d, poses[a], poses[b])
            assert abs(ang - max_angle) >= TIE, (name, d, "an angle within 1e-9 of max_angle")
            dropped += not ang <= max_angle
        assert dropped > 0 and red.any()


def test_abi_and_bindings_cover_the_removals():
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    L = C.CDLL(lib.LIB_PATH)
    assert "spg_graph_select_removals" in lib.SYMBOLS and hasattr(L, "spg_graph_select_removals")
    assert C.sizeof(abi.RemovalStats) == 56
    assert list(abi.RemovalStats().asdict()) == ["n_cells", "max_cell_population", "table_slots", "n_live", "n_forced", "n_kept", "n_removed", "rounds",
                                                  "pairs_tested", "device_seconds"]
    assert abi.RemovalStats.pairs_tested.offset == 40 and abi.RemovalStats.device_seconds.offset == 48
    assert callable(GraphWrapperHIP.selectRemovals)
    hdr = open(os.path.join(ROOT, "include", "spg.h")).read()
    assert "spg_removal_stats" in hdr and "spg_graph_select_removals" in hdr and "lexicographically first maximal independent set" in hdr
    assert "selectRemovals" in open(os.path.join(ROOT, "include", "spg_graph_wrapper.hpp")).read()
    assert "hip_select_removals" in open(os.path.join(ROOT, "tools", "asan_stubs.cpp")).read()
    assert "spg_removals.inc" in open(os.path.join(PKG, "csrc", "Makefile")).read()


def test_removals_check_arguments_before_the_backend():
    """On an injected (CPU) context: radius <= 0 / inf / NaN, max_angle = NaN, an unknown and a repeated keep id, a NaN
    priority and an active stepwise marginalisation are SPG_EINVAL with the offending value or id in the text; no and one
    live vertex return 0; a call that would compute is SPG_ESTATE (no CPU fallback); the Python layer raises."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    sub = _small()
    ictx = oracle_lib.injected_context()
    a = GraphWrapperHIP.from_dict(sub, ctx=ictx)
    L = a.L
    ids = np.sort(np.asarray(sub["ids"], np.int32))
    err = lambda: L.spg_last_error(ictx.h).decode()  # noqa: E731
    st = abi.RemovalStats()

    def call(radius=1.0, max_angle=0.0, keep=None, prio=None, h=a.h):
        kp = None if keep is None else np.ascontiguousarray(keep, np.int32)
        pp = None if prio is None else np.ascontiguousarray(prio, np.float64)
        return L.spg_graph_select_removals(h, radius, max_angle, None if kp is None else kp.ctypes.data_as(_i32p), 0 if kp is None else len(kp),
                                           None if pp is None else pp.ctypes.data_as(_f64p), None, None, None, 0, C.byref(st))
    assert call() == ESTATE and "HIP backend" in err() and "spg_graph_select_removals" in err()
    assert call(keep=ids[:3], prio=np.arange(len(ids), dtype=np.float64)) == ESTATE
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert call(radius=bad) == EINVAL and "radius" in err()
    assert call(max_angle=np.nan) == EINVAL and "max_angle" in err()
    assert call(keep=[int(ids[0]), 999999]) == EINVAL and "999999" in err() and "keep 1" in err()
    assert call(keep=[int(ids[0]), int(ids[1]), int(ids[0])]) == EINVAL and "twice" in err() and str(int(ids[0])) in err() and "keep 2" in err()
    prio = np.zeros(len(ids))
    prio[4] = np.nan
    assert call(prio=prio) == EINVAL and "priority" in err() and f"vertex {int(ids[4])} " in err()
    prio[4] = np.inf                                                  # infinite priorities are values like any other
    assert call(prio=prio) == ESTATE
    assert L.spg_graph_select_removals(None, 1.0, 0.0, None, 0, None, None, None, None, 0, None) == EINVAL
    one = GraphWrapperHIP(ctx=ictx, pose_dim=3)
    assert call(h=one.h) == 0 and st.n_live == 0                      # no vertex
    assert call(h=one.h, keep=[7]) == EINVAL and "vertex 7 " in err()
    one.addVertex(7, [0.0, 0.0, 0.0])
    assert call(h=one.h) == 0 and (st.n_live, st.n_kept, st.n_removed, st.rounds) == (1, 1, 0, 0)
    assert call(h=one.h, keep=[7]) == 0 and st.n_forced == 1
    g, which, opts, *_ = util.load_golden("intel_nfr_tree_sp3")
    sub2, w = util.prefix_graph(g, which, 30)
    b = GraphWrapperHIP.from_dict(sub2, ctx=ictx)
    b.begin(w, opts, 0, 1)
    assert call(h=b.h) == EINVAL and "active" in err()
    with pytest.raises(SpgError, match="HIP backend"):
        a.selectRemovals(1.0)
    with pytest.raises(SpgError, match="radius"):
        a.selectRemovals(0.0)
    with pytest.raises(SpgError, match="999999"):
        a.selectRemovals(1.0, keep=[999999])
    with pytest.raises(SpgError, match="priority"):
        a.selectRemovals(1.0, priority={int(i): (np.nan if k == 2 else 1.0) for k, i in enumerate(ids)})
    with pytest.raises(ValueError, match="priority"):
        a.selectRemovals(1.0, priority=[1.0, 2.0])
    with pytest.raises(ValueError, match="priority"):
        a.selectRemovals(1.0, priority={int(ids[0]): 1.0})
    with pytest.raises(ValueError, match="priority"):
        a.selectRemovals(1.0, priority="middle")
    for p in ("oldest", "newest", None):
        with pytest.raises(SpgError, match="HIP backend"):
            a.selectRemovals(1.0, priority=p)
    rem, rep, rd, s = one.selectRemovals(1.0, stats=True)
    assert rem.shape == rep.shape == rd.shape == (0,) and rem.dtype == rep.dtype == np.int32 and s["n_kept"] == 1


def _build_demo(tmp_path):
    exe = str(tmp_path / "removals_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "removals_demo.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_removals_demo_compiles(tmp_path):
    out = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr


# ------------------------------------------------------------------------------------------------------- GPU
def _check(hg, d, ids, poses, radius, max_angle, keep, prio, table, what):
    """one device run (twice) against the reference; returns (removed, representative, rep_dist, stats, ref)"""
    ref = rf.select(d, ids, poses, radius, max_angle, keep, prio, table=table)
    rem, rep, rd, s = hg.selectRemovals(radius, max_angle, keep, prio, stats=True)
    again = hg.selectRemovals(radius, max_angle, keep, prio)
    print(f"{what}: {len(ref['removed'])} of {len(ids)} removed, {s['rounds']} rounds, {s['pairs_tested']} tests")
    assert rem.dtype == np.int32 and np.array_equal(rem, ref["removed"]), (what, len(rem), len(ref["removed"]))
    assert np.array_equal(rep, ref["representative"]), what
    assert rd.tobytes() == ref["rep_dist"].tobytes(), what
    for x, y in zip((rem, rep, rd), again):
        assert x.tobytes() == y.tobytes(), what
    cells = {tuple(c) for c in np.floor(poses[:, :pr.dim(d)] / radius).astype(np.int64)}
    assert s["n_cells"] == len(cells) and s["table_slots"] >= 2 * len(ids) and s["table_slots"] & (s["table_slots"] - 1) == 0
    assert (s["n_live"], s["n_forced"], s["n_removed"], s["n_kept"]) == (len(ids), len(keep), len(rem), len(ids) - len(rem)), what
    assert s["device_seconds"] > 0 and (s["rounds"] >= 1) == (len(keep) < len(ids)) and s["rounds"] <= len(ids)
    return rem, rep, rd, s, ref


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_selection_equals_the_reference(d, hip_ctx):
    """Every fixture in hash order, "oldest", "newest" and a random priority with repeated values, with no, five and two
    mutually redundant forced vertices: removed and representative equal, rep_dist bit for bit, two calls the same bytes."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    for name, *_ in _cases(d):
        g, ids, poses, radius, max_angle, table = _case(d, name)
        hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
        for order in ORDERS:
            for which in KEEPS:
                keep = _keep(ids, table[0], which)
                rem, rep, rd, s, ref = _check(hg, d, ids, poses, radius, max_angle, keep, _priority(ids, order), table,
                                              f"SE{2 if d == 3 else 3} {name}, {order}, keep {which}")
                if which == "pair":
                    assert not set(keep) & set(rem.tolist()) and table[0][ids.index(keep[0]), ids.index(keep[1])]
                if name == "one cell":
                    assert s["max_cell_population"] == 300 and s["n_cells"] == 1 and s["n_kept"] == max(len(keep), 1)
                if name == "lattice, unjittered" and which == "none":
                    assert (rd == radius).sum() > 0                                  # the <= at exactly the radius
        if name == "two clusters":
            assert np.abs(np.floor(poses[:, 0] / radius)).min() > 9e5              # cell coordinates near the 21-bit limit
    # a dict and the strings are the arrays they stand for
    g, ids, poses, radius, max_angle, table = _case(d, "cloud")
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    by_dict = hg.selectRemovals(radius, priority={i: -float(i) for i in ids})
    by_name = hg.selectRemovals(radius, priority="oldest")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(by_dict, by_name))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_long_dependency_chain(d, hip_ctx):
    """256 poses on a line at spacing 0.2, radius 0.5, ids along the line: in "oldest" order every decision hangs on the one
    before it (kept, removed, removed, kept, ...), the deepest chain this size allows; the result equals the reference in
    1 <= rounds <= depth + 1. The same graph in hash order: rounds <= its own depth, and <= the depth of "oldest"."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    pos = np.zeros((256, pr.dim(d)))
    pos[:, 0] = 0.2 * np.arange(256)
    g = _graph(d, pos, seed=8, ids=np.arange(256))
    ids, poses = _sorted_graph(g)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    table = rf.redundancy(d, poses, 0.5)
    out = {}
    for order in ("oldest", "hash"):
        prio = _priority(ids, order)
        rem, rep, rd, s, ref = _check(hg, d, ids, poses, 0.5, 0.0, [], prio, table, f"SE{2 if d == 3 else 3} line, {order}")
        _, depth = rf.rounds(table[0], ref["order"], 0)
        print(f"line, {order}: depth {depth}, rounds {s['rounds']}")
        assert 1 <= s["rounds"] <= depth + 1
        out[order] = (s["rounds"], depth, rem)
    assert out["oldest"][2].tolist() == [i for i in range(256) if i % 3] and out["oldest"][1] >= 2 * 85
    assert out["hash"][0] <= out["hash"][1] and out["hash"][0] <= out["oldest"][1]


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
    rem, rep, rd, s = hg.selectRemovals(0.3, stats=True)
    np.savez(os.path.join(sys.argv[3], "table.npz"), rem=rem, rep=rep, rd=rd, slots=s["table_slots"])
    print("ran", s["table_slots"])
except SpgError as e:
    print("refused", e)
'''


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_forced_small_table_gives_the_same_removals(d, tmp_path, hip_ctx):
    """SPG_PROPOSE_TABLE_BITS at the smallest admissible value (a table more than half full) in a fresh process returns the
    bytes of the default table; one bit less is SPG_ECAPACITY."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    hg = GraphWrapperHIP.from_dict(_table_cloud(d), ctx=hip_ctx)
    rem, rep, rd, s = hg.selectRemovals(0.3, stats=True)
    cells = s["n_cells"]
    bits = int(np.ceil(np.log2(cells)))
    assert 2 ** (bits - 1) < cells <= 2 ** bits < s["table_slots"] and len(rem) > 100
    script = tmp_path / "table_child.py"
    script.write_text(TABLE_CHILD)
    out = subprocess.run([sys.executable, str(script), ROOT, str(bits), str(tmp_path), str(d)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ran" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    got = np.load(str(tmp_path / "table.npz"))
    assert int(got["slots"]) == 2 ** bits
    for key, want in (("rem", rem), ("rep", rep), ("rd", rd)):
        assert got[key].tobytes() == want.tobytes(), key
    out = subprocess.run([sys.executable, str(script), ROOT, str(bits - 1), str(tmp_path), str(d)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "refused" in out.stdout and "occupied cells" in out.stdout and f"code {ECAPACITY}" in out.stdout, \
        out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_edges_of_the_domain(d, hip_ctx):
    """No, one and two live vertices; every vertex forced; a radius below every distance removes nothing, one above the
    whole graph keeps one unforced vertex, the first of the order; a pose that is not finite is SPG_EINVAL with its id, one
    whose cell coordinate does not fit 21 bits SPG_ECAPACITY with its id."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    k = pr.dim(d)
    none = GraphWrapperHIP(ctx=hip_ctx, pose_dim=d)
    assert len(none.selectRemovals(1.0)[0]) == 0
    one = GraphWrapperHIP.from_dict(_graph(d, np.zeros((1, k)), seed=1), ctx=hip_ctx)
    assert len(one.selectRemovals(1.0)[0]) == 0
    pos = np.zeros((2, k))
    pos[1, 0] = 0.3
    two = GraphWrapperHIP.from_dict(_graph(d, pos, seed=2, ids=[4, 9], chain=False), ctx=hip_ctx)
    rem, rep, rd, s = two.selectRemovals(1.0, priority="oldest", stats=True)
    assert (rem.tolist(), rep.tolist(), rd.tolist()) == ([9], [4], [0.3]) and s["rounds"] in (1, 2) and s["n_kept"] == 1
    rem, rep, rd = two.selectRemovals(1.0, priority="newest")
    assert (rem.tolist(), rep.tolist(), rd.tolist()) == ([4], [9], [0.3])
    assert len(two.selectRemovals(0.2)[0]) == 0
    rem, rep, rd, s = two.selectRemovals(1.0, keep=[9, 4], stats=True)
    assert len(rem) == 0 and (s["n_forced"], s["n_kept"], s["rounds"]) == (2, 2, 0)
    g = _cloud(d, 200, 1.0, 9)
    ids, poses = _sorted_graph(g)
    cloud = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    rem, rep, rd, s = cloud.selectRemovals(0.5, keep=ids, stats=True)                  # everything forced
    assert len(rem) == 0 and (s["n_forced"], s["n_kept"], s["rounds"]) == (200, 200, 0)
    dist = pr.distance_table(d, poses)
    below = 0.5 * dist[dist > 0].min()
    rem, rep, rd, s = cloud.selectRemovals(below, stats=True)
    assert len(rem) == 0 and s["n_kept"] == 200 and s["rounds"] == 1
    above = 2.0 * dist.max()
    rem, rep, rd, s = cloud.selectRemovals(above, stats=True)
    first = ids[rf.order_of(ids)[0][0]]
    assert s["n_kept"] == 1 and first not in rem.tolist() and set(rep.tolist()) == {first} and len(rem) == 199
    far = _two_clusters(d, centre=6e5)
    hg = GraphWrapperHIP.from_dict(far, ctx=hip_ctx)
    with pytest.raises(SpgError, match="21 bits") as e:
        hg.selectRemovals(0.5)
    fids, fposes = _sorted_graph(far)
    bad_id = next(i for i, p in zip(fids, fposes) if not -2 ** 20 <= np.floor(p[0] / 0.5) < 2 ** 20)
    assert f"vertex {bad_id} " in str(e.value) and f"code {ECAPACITY}" in str(e.value) and "spg_graph_select_removals" in str(e.value)
    assert len(hg.selectRemovals(1.0)[0]) > 0                                            # the same poses fit at radius 1
    for bad in (np.nan, np.inf):
        pos3 = np.zeros((3, k))
        pos3[:, 0] = [0.0, 0.3, 0.6]
        g3 = _graph(d, pos3, seed=3, ids=[4, 8, 9], chain=False)
        g3["poses"][1, k - 1] = bad
        with pytest.raises(SpgError, match="not finite") as e:
            GraphWrapperHIP.from_dict(g3, ctx=hip_ctx).selectRemovals(1.0)
        assert "vertex 8 " in str(e.value) and f"code {EINVAL}" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["intel_nfr_tree_sp3", "sphere_glc_tree"])
def test_marginalised_graphs(case, hip_ctx):
    """Every second vertex marginalised: the live ids are non-contiguous and (under GLC) n-ary edges are present; the
    selection sees the live vertices alone and equals the reference, with and without max_angle."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, which, opts, *_ = util.load_golden(case)
    sub, _ = util.prefix_graph(g, which, 80)
    d = sub["pose_dim"]
    hg = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx, useGLC=opts.algorithm == abi.ALG_GLC)
    w = np.asarray(sub["ids"], np.int32)[1:-1:2]
    st = hg.marginalizeNoOptimize(w, opts)
    assert st["n_bad_status"] == 0 and st["n_removed"] == len(w)
    ids, poses = hg.vertices()
    o = np.argsort(ids)
    ids, poses = [int(i) for i in ids[o]], poses[o]
    assert not set(ids) & set(w.tolist()) and np.any(np.diff(ids) > 1)
    radius = float(np.sort(pr.distance_table(d, poses), axis=1)[:, 4].mean()) * 1.0000001
    for max_angle, order, keep in ((0.0, "hash", []), (0.0, "newest", [ids[0]]), (1.0, "oldest", [ids[-1], ids[0]])):
        table = rf.redundancy(d, poses, radius, max_angle)
        if max_angle > 0:
            for a, b in zip(*np.nonzero(np.triu(table[1] <= radius, 1))):
                assert abs(pr.rotation_angle(d, poses[a], poses[b]) - max_angle) >= TIE
        rem, *_ = _check(hg, d, ids, poses, radius, max_angle, keep, _priority(ids, order), table, f"{case} marginalised, {order}")
        assert len(rem) > 5


@pytest.mark.gpu
def test_selection_feeds_the_marginalisation_end_to_end(hip_ctx):
    """The first SMALL graph of the covariance tests: selectRemovals with the fixed vertex forced, its list into
    marginalizeNoOptimize (NFR Tree); the live ids are exactly the kept set, a second selection with the same arguments
    removes nothing, and the KLD of the sparsified graph against the baseline is finite."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    case, n = SMALL[0]
    g, which, opts, *_ = util.load_golden(case)
    assert opts.algorithm != abi.ALG_GLC
    sub, _ = util.prefix_graph(g, which, n)
    d = sub["pose_dim"]
    base = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx)
    sp = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx)
    ids, poses = sp.vertices()
    fixed = int(ids.min())
    radius = float(np.sort(pr.distance_table(d, poses), axis=1)[:, 3].mean())
    rem, rep, rd, s = sp.selectRemovals(radius, keep=[fixed], stats=True)
    assert 0 < len(rem) < len(ids) and fixed not in rem.tolist() and np.all(rd <= radius)
    st = sp.marginalizeNoOptimize(rem, opts)
    assert st["n_removed"] == len(rem)
    live = np.sort(sp.vertices()[0])
    assert np.array_equal(live, np.setdiff1d(ids, rem)) and len(live) == s["n_kept"]
    again, _, _, s2 = sp.selectRemovals(radius, keep=[fixed], stats=True)
    assert len(again) == 0 and s2["n_removed"] == 0 and s2["n_live"] == len(live)
    kld = base.kullbackLeibler(sp)
    print(f"{case}[{n}]: {len(rem)} of {len(ids)} removed at radius {radius:.3f} in {s['rounds']} rounds, KLD {kld:.4g}")
    assert np.isfinite(kld)
