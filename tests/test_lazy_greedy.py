"""Lazy greedy selection and pruning (SPG_GREEDY_LAZY): spg_graph_select_candidates / _prune_candidates without
the joint covariance of the endpoints — round 0 from the per-pair blocks, each round's covariance columns solved on demand
into a column cache. The recurrence, the references (tests/select_ref.py, tests/prune_ref.py) and the bounds are those of
tests/test_candidate_selection.py (_single_bounds, (t + 1) single) and tests/test_edge_pruning.py (_bounds): their premise,
a covariance error of 1e-9 max|Sigma|, covers column-solved blocks as it covers pairCovariances. Nothing is widened here.

CPU: the two context symbols, the method / lookahead contract, zero stats, argument errors unchanged under LAZY, the
46 000 rule per method on an injected context, the column-cache planner (tests/cpp/lazy_greedy_plan_demo.cpp, plain and
with -fsanitize=address,undefined, as a stand-alone program). GPU: sequences and values on the small fixtures with
lookahead 1 and 0, stop rules and sizes, lookahead and a forced two-strip cache change cost but not results, a graph past
the joint bound (7 999 SE3 endpoints), and that nothing else moved. Measured figures: DESIGN 7.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sparsifyposegraph_amd import abi, g2o_io, lib
from sparsifyposegraph_amd.lib import SpgError
from tests import oracle_lib
from tests import prune_ref as pr
from tests import relative_ref as rr
from tests import select_ref as sr
from tests import test_candidate_selection as tcs
from tests import test_edge_pruning as tep
from tests.test_candidate_selection import _at, _fids, _poses, _single_bounds
from tests.test_covariance_blocks import _oracle_of, _small
from tests.test_relative_covariance import _far_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")
CSRC = os.path.join(PKG, "csrc")
_f64p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
EINVAL, ECAPACITY, ESTATE = -1, -4, -7
K = 8
LOOKAHEADS = (1, 0)


@pytest.fixture
def lazy(hip_ctx):
    """sets a greedy method on the shared context; JOINT, the default, is restored afterwards"""
    def use(method, lookahead=0):
        hip_ctx.set_greedy_method(method, lookahead)
    yield use
    hip_ctx.set_greedy_method(abi.GREEDY_JOINT, 0)
    os.environ.pop("SPG_GREEDY_CACHE_STRIPS", None)


def _accounted(ij_or_pairs, chosen, fid, st):
    """column_vertices + column_hits covers every non-fixed endpoint of every chosen candidate"""
    need = sum(int(a != fid) + int(b != fid) for a, b in (ij_or_pairs[i] for i in chosen))
    assert st["column_vertices"] + st["column_hits"] >= need and st["column_hits"] <= need, (st, need)
    if st["lookahead"] == 1:
        assert st["column_vertices"] + st["column_hits"] == need, (st, need)


# ------------------------------------------------------------------------------------------------------- CPU
def test_abi_and_bindings_cover_the_greedy_method():
    from sparsifyposegraph_amd.graph import GraphWrapperHIP  # noqa: F401
    L = C.CDLL(lib.LIB_PATH)
    for name in ("spg_ctx_set_greedy_method", "spg_ctx_greedy_stats"):
        assert name in lib.SYMBOLS and hasattr(L, name)
    assert (abi.GREEDY_JOINT, abi.GREEDY_LAZY, abi.GREEDY_AUTO) == (0, 1, 2)
    assert C.sizeof(abi.GreedyStats) == 56
    hdr = open(os.path.join(ROOT, "include", "spg.h")).read()
    assert "SPG_GREEDY_JOINT = 0, SPG_GREEDY_LAZY = 1, SPG_GREEDY_AUTO = 2" in hdr
    wrap = open(os.path.join(ROOT, "include", "spg_graph_wrapper.hpp")).read()
    assert "setGreedyMethod" in wrap and "greedyStats" in wrap
    ictx = oracle_lib.injected_context()
    Li = ictx.L
    zero = {k: 0 for k, _ in abi.GreedyStats._fields_}
    assert ictx.greedy_stats() == zero
    for method in (abi.GREEDY_JOINT, abi.GREEDY_LAZY, abi.GREEDY_AUTO):
        for look in (0, 1, 5, 1000):
            assert Li.spg_ctx_set_greedy_method(ictx.h, method, look) == 0
    for method, look in ((-1, 0), (3, 0), (abi.GREEDY_LAZY, -1), (abi.GREEDY_JOINT, -7)):
        assert Li.spg_ctx_set_greedy_method(ictx.h, method, look) == EINVAL
    assert Li.spg_ctx_set_greedy_method(None, 0, 0) == EINVAL and Li.spg_ctx_greedy_stats(ictx.h, None) == EINVAL
    with pytest.raises(SpgError):
        ictx.set_greedy_method(7)
    assert ictx.greedy_stats() == zero


def test_argument_errors_are_unchanged_under_lazy():
    """With LAZY set on an injected context the argument errors of both calls come before the backend, as in JOINT; a call
    that would compute is SPG_ESTATE."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    sub = _small()
    ictx = oracle_lib.injected_context()
    ictx.set_greedy_method(abi.GREEDY_LAZY, 0)
    a = GraphWrapperHIP.from_dict(sub, ctx=ictx)
    D = 3
    e0 = [int(x) for x in sub["edge_ij"][0]]
    pairs = np.array([e0, [e0[1], e0[0]]], np.int32)
    rec = np.ascontiguousarray(np.tile(sub["edge_data"][0], (2, 1)))
    with pytest.raises(SpgError, match="HIP backend"):
        a.selectCandidates(pairs, rec[:, :D], rec[:, D:], 2)
    with pytest.raises(SpgError, match="same"):
        a.selectCandidates([[e0[0], e0[0]]], rec[:1, :D], rec[:1, D:], 1)
    with pytest.raises(SpgError, match="999999"):
        a.selectCandidates([[e0[0], 999999]], rec[:1, :D], rec[:1, D:], 1)
    with pytest.raises(SpgError, match="negative"):
        a.selectCandidates(pairs, rec[:, :D], rec[:, D:], -1)
    with pytest.raises(SpgError, match="fixed vertex"):
        a.selectCandidates(pairs, rec[:, :D], rec[:, D:], 1, fixed_id=999999)
    r2 = rec.copy()
    r2[1, 1] = np.nan
    with pytest.raises(SpgError, match="finite"):
        a.selectCandidates(pairs, r2[:, :D], r2[:, D:], 1)
    assert len(a.selectCandidates(pairs, rec[:, :D], rec[:, D:], 0)["selected"]) == 0
    idx = np.array([0, 2, 5], np.int32)
    with pytest.raises(SpgError, match="HIP backend"):
        a.pruneCandidates(idx, 2)
    with pytest.raises(SpgError, match="listed twice"):
        a.pruneCandidates([1, 1], 1)
    with pytest.raises(SpgError, match="out of range"):
        a.pruneCandidates([0, a.numEdges() + 3], 1)
    with pytest.raises(SpgError, match="negative"):
        a.pruneCandidates(idx, -1)
    with pytest.raises(SpgError, match="fixed vertex"):
        a.pruneCandidates(idx, 1, fixed_id=999999)
    assert len(a.pruneCandidates(idx, 0)["pruned"]) == 0
    assert ictx.greedy_stats()["rounds"] == 0


def test_the_joint_bound_applies_to_joint_alone():
    """15 999 SE2 endpoints (47 997 > 46 000 variables) on an injected context: JOINT answers SPG_ECAPACITY, LAZY and AUTO
    get past that rule to SPG_ESTATE (no HIP), for both calls; the size query answers in every mode."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_manhattan(n_poses=16000, side=130)
    ictx = oracle_lib.injected_context()
    hg = GraphWrapperHIP.from_dict(g, ctx=ictx)
    ids = [int(i) for i in g["ids"]]
    L = hg.L
    n = 15999
    star = np.ascontiguousarray([(ids[0], v) for v in ids[1:n + 1]], np.int32)
    rec = np.ascontiguousarray(np.tile(g["edge_data"][0], (n, 1)))
    e = hg.edges()
    chain = np.flatnonzero(e["kind"] == abi.EDGE_BINARY).astype(np.int32)
    assert len({int(v) for v in g["edge_ij"].ravel()}) >= n + 1
    sel, cg = np.zeros(4, np.int32), np.zeros(4)
    cl, ck = np.zeros(4), np.zeros(4)
    f = lambda x: x.ctypes.data_as(_f64p)  # noqa: E731
    i = lambda x: x.ctypes.data_as(_i32p)  # noqa: E731

    def select(cap=4):
        return L.spg_graph_select_candidates(hg.h, -1, i(star), f(rec), n, 4, 0.0, 0.0, i(sel), f(cg), cap, None, None, None)

    def prune(cap=4):
        return L.spg_graph_prune_candidates(hg.h, -1, i(chain), len(chain), 4, 0.0, 0.0, 0.0, i(sel), f(cl), f(ck), cap, None, None, None, None)
    for method, want in ((abi.GREEDY_JOINT, ECAPACITY), (abi.GREEDY_LAZY, ESTATE), (abi.GREEDY_AUTO, ESTATE)):
        ictx.set_greedy_method(method, 0)
        assert select() == want and prune() == want, method
        msg = L.spg_last_error(ictx.h).decode()
        assert ("46k" in msg) if want == ECAPACITY else ("HIP backend" in msg)
        if method != abi.GREEDY_JOINT:
            assert select(cap=0) == 4 and prune(cap=0) == 4


def test_column_cache_planner_plain_and_sanitized(tmp_path):
    """tests/cpp/lazy_greedy_plan_demo.cpp against csrc/spg_greedy_plan.hpp, a stand-alone program: scripted ranked lists
    give the expected solve sets, strips, hits and evictions; two strips serve every round; fixed endpoints get no strip.
    Built and run twice: plainly, and under AddressSanitizer + UBSan."""
    src = os.path.join(ROOT, "tests", "cpp", "lazy_greedy_plan_demo.cpp")
    for name, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("lazy_greedy_plan_demo_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", *flags, "-I" + CSRC, "-o", exe, src])
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip() == "ok", (name, out.stdout, out.stderr)


# ------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case,n", tcs.CASES)
def test_lazy_selection_sequence_and_gains(case, n, hip_ctx, lazy):
    """The 61 candidates of test_candidate_selection, k = 8, before and after the case's marginalisation, both gauges, LAZY
    with lookahead 1 and 0: the reference's sequence exactly, cond_gain[t] and final_gain within (t + 1) single bounds, the
    statuses of the joint run, of the three identical copies the lowest index chosen and the two others bit-identical, the
    stats. One numpy reference per graph and gauge serves every run.
    Measured on an MI355X, worst error / bound: 3.5e-6 (intel), 1.6e-7 (sphere), 4.7e-6 (manhattan GLC Tree), the same with
    both lookaheads."""
    from tests.test_relative_covariance import _small_graphs
    sub, graphs, kept = _small_graphs(case, n, hip_ctx)
    d = sub["pose_dim"]
    worst = 0.0
    same = (tcs.I_COPY, tcs.I_COPY + 1, tcs.I_COPY + 2)
    for hg, og in graphs:
        ids = [int(i) for i in hg.vertices()[0]]
        for fid in _fids(ids, kept):
            Sig = np.linalg.inv(og.information(fid))
            ij, meas, info = tcs._small_candidates(d, hg, sub, fid, Sig, tcs.GRADE)
            ref, single, _ = tcs._reference(d, hg, fid, Sig, ij, meas, info, K)
            lazy(abi.GREEDY_JOINT)
            joint = hg.selectCandidates(ij, meas, info, K, fixed_id=fid)
            assert hip_ctx.greedy_stats()["method"] == abi.GREEDY_JOINT and hip_ctx.greedy_stats()["rounds"] == K
            for look in LOOKAHEADS:
                lazy(abi.GREEDY_LAZY, look)
                got = hg.selectCandidates(ij, meas, info, K, fixed_id=fid)
                what = f"lazy select {case}[{n}] {'after' if hg is graphs[1][0] else 'before'} fixed {fid} lookahead {look}"
                worst = max(worst, tcs._check_against(ref, single, got, tcs.N_CAND, what))
                assert np.array_equal(got["status"], joint["status"]) and got["status"][tcs.I_BAD] == abi.CAND_INFO_NOT_PD
                copies = [i for i in got["selected"] if i in same]
                left = [i for i in same if i not in copies]
                assert copies == list(same[:len(copies)]) and len(left) == 2
                assert np.isfinite(got["final_gain"][left[0]]) and got["final_gain"][left[0]] == got["final_gain"][left[1]]
                s, st = hg.last_covariance_stats, hip_ctx.greedy_stats()
                assert s["rounds"] == K and 0 < s["select_seconds"] < s["device_seconds"]
                assert s["endpoints"] == len({int(v) for v in ij.ravel()} - {fid})
                assert st["method"] == abi.GREEDY_LAZY and st["rounds"] == K and st["refactorised"] == 1 and st["cache_bytes"] > 0
                assert st["lookahead"] == (1 if look == 1 else (5 if d == 6 else 10)) and 0 < st["round_solve_seconds"] < s["select_seconds"]
                _accounted(ij, got["selected"], fid, st)
    print(f"lazy select {case}[{n}]: worst error / bound {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", tep.CASES)
def test_lazy_pruning_sequence_and_values(case, n, hip_ctx, lazy):
    """The 40 graded edges of test_edge_pruning are added and are the candidates, k = 8, before and after the case's
    marginalisation, both gauges, LAZY with lookahead 1 and 0: the reference's sequence exactly, cond_loss[t], kld[t],
    final_loss and final_margin within their bounds, the statuses, the stats; column_hits > 0 with a full panel.
    Measured on an MI355X, worst error / bound: 9.2e-6 (intel), 2.7e-7 (sphere), 1.25e-4 (manhattan GLC Tree), the joint
    mode's figures."""
    from tests.test_relative_covariance import _small_graphs
    sub, graphs, kept = _small_graphs(case, n, hip_ctx)
    d = sub["pose_dim"]
    worst = 0.0
    for hg, og in graphs:
        ids = [int(i) for i in hg.vertices()[0]]
        for fid in _fids(ids, kept):
            H0 = og.information(fid)
            ij, meas, info, rank, T, H1, Sig1 = tep._problem(d, hg, fid, H0)
            ref = pr.greedy_sigma(Sig1, T, [True] * tep.N_ADD, K)
            single = _single_bounds(d, T, Sig1)
            before = tep._edge_rows(hg.edges())
            idx = tep._add_list(hg, ij, meas, info)
            lazy(abi.GREEDY_JOINT)
            joint = hg.pruneCandidates(idx, K, fixed_id=fid)
            for look in LOOKAHEADS:
                lazy(abi.GREEDY_LAZY, look)
                got = hg.pruneCandidates(idx, K, fixed_id=fid)
                what = f"lazy prune {case}[{n}] {'after' if hg is graphs[1][0] else 'before'} fixed {fid} lookahead {look}"
                worst = max(worst, tep._check_against(d, ref, single, got, what))
                assert np.array_equal(got["status"], joint["status"])
                s, st = hg.last_covariance_stats, hip_ctx.greedy_stats()
                assert s["rounds"] == K and 0 < s["prune_seconds"] < s["device_seconds"] and s["columns"] == 0   # every pair is an edge
                assert s["endpoints"] == len({int(v) for v in ij.ravel()} - {fid})
                assert st["method"] == abi.GREEDY_LAZY and st["rounds"] == K and st["refactorised"] == 1
                _accounted(ij, got["pruned"], fid, st)
                if look == 0:
                    assert st["column_hits"] > 0 and st["rhs_batches"] < K, st
                else:
                    assert st["rhs_batches"] <= K
            hg.removeEdges(idx)
            assert tep._edge_rows(hg.edges()) == before
    print(f"lazy prune {case}[{n}]: worst error / bound {worst:.2e}")


@pytest.mark.gpu
def test_lazy_stop_rules_and_sizes(hip_ctx, lazy):
    """synth_manhattan(400) with 300 candidates (two workgroups of partials, a ranked list that spans them), k = 5, LAZY:
    the reference's sequence; the min_gain / max_loss / max_kld stops; k > n; n = 1 with k = 1; an edge to the fixed vertex;
    the 4-cycle's dynamic bridge; greedy_stats.rounds equals the rounds of the call and the columns account for every
    non-fixed endpoint of every chosen candidate."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_manhattan(n_poses=400, side=20)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    fid = int(g["ids"][0])
    H0 = _oracle_of(hg).information(fid)
    Sig = np.linalg.inv(H0)
    lazy(abi.GREEDY_LAZY, 0)
    # selection
    ij, meas, info = tcs._manhattan_candidates(g, hg)
    ref, single, _ = tcs._reference(3, hg, fid, Sig, ij, meas, info, 5)
    got = hg.selectCandidates(ij, meas, info, 5, fixed_id=fid)
    tcs._check_against(ref, single, got, 300, "lazy manhattan 300")
    st = hip_ctx.greedy_stats()
    assert st["rounds"] == 5 == hg.last_covariance_stats["rounds"] and st["method"] == abi.GREEDY_LAZY
    _accounted(ij, got["selected"], fid, st)
    assert got["status"][7] == abi.CAND_INFO_NOT_PD and np.isnan(got["final_gain"][7])
    mid = 0.5 * (ref["cond_gain"][2] + ref["cond_gain"][3])
    ref3, _, _ = tcs._reference(3, hg, fid, Sig, ij, meas, info, 5, min_gain=mid)
    got3 = hg.selectCandidates(ij, meas, info, 5, min_gain=mid, fixed_id=fid)
    assert len(got3["selected"]) == 3 and hg.last_covariance_stats["rounds"] == 3 and hip_ctx.greedy_stats()["rounds"] == 3
    tcs._check_against(ref3, single, got3, 300, "lazy manhattan 300, min_gain")
    few = [5, 6, 7, 8, 9]
    refk, _, _ = tcs._reference(3, hg, fid, Sig, ij[few], meas[few], info[few], 9)
    gotk = hg.selectCandidates(ij[few], meas[few], info[few], 9, fixed_id=fid)
    assert len(gotk["selected"]) == 4 and np.array_equal(gotk["selected"], refk["selected"]) and hip_ctx.greedy_stats()["rounds"] == 4
    assert np.array_equal(gotk["status"], [3, 3, 1, 3, 3]) and np.all(np.isnan(gotk["final_gain"]))
    got1 = hg.selectCandidates(ij[:1], meas[:1], info[:1], 1, fixed_id=fid)
    assert got1["selected"].tolist() == [0] and abs(got1["cond_gain"][0] - ref["rounds"][0][0]) <= single[0]
    # pruning
    d = 3
    far, pmeas, pinfo, T, ok, H1 = tep._manhattan_list(hg, fid, H0)
    idx = tep._add_list(hg, far, pmeas, pinfo)
    Sig1 = np.linalg.inv(H1)
    psingle = _single_bounds(d, T, Sig1)
    psingle[7] = np.inf
    pref = pr.greedy_sigma(Sig1, T, ok, 5)
    pgot = hg.pruneCandidates(idx, 5, fixed_id=fid)
    tep._check_against(d, pref, psingle, pgot, "lazy manhattan 300")
    st = hip_ctx.greedy_stats()
    assert st["rounds"] == 5 == hg.last_covariance_stats["rounds"]
    _accounted(far, pgot["pruned"], fid, st)
    assert pgot["status"][7] == abi.PRUNE_INFO_NOT_PD and pgot["status"][5] == abi.PRUNE_KEPT and np.isfinite(pgot["final_loss"][5])
    mid = 0.5 * (pref["cond_loss"][2] + pref["cond_loss"][3])
    pgot3 = hg.pruneCandidates(idx, 5, max_loss=mid, fixed_id=fid)
    assert pgot3["pruned"].tolist() == [0, 1, 2] and hg.last_covariance_stats["rounds"] == 3 and hip_ctx.greedy_stats()["rounds"] == 3
    tep._check_against(d, pr.greedy_sigma(Sig1, T, ok, 5, max_loss=mid), psingle, pgot3, "lazy manhattan 300, max_loss")
    midk = 0.5 * (pref["kld"][1] + pref["kld"][2])
    pgotk = hg.pruneCandidates(idx, 5, max_kld=midk, fixed_id=fid)
    assert pgotk["pruned"].tolist() == [0, 1] and np.array_equal(pgotk["kld"], pgot["kld"][:2])
    fewp = idx[[5, 6, 7, 8, 9]]
    pgotn = hg.pruneCandidates(fewp, 9, fixed_id=fid)
    assert len(pgotn["pruned"]) == 4 and sorted(pgotn["pruned"].tolist()) == [0, 1, 3, 4] and np.array_equal(pgotn["status"], [3, 3, 1, 3, 3])
    assert np.all(np.isnan(pgotn["final_loss"])) and np.all(np.diff(pgotn["kld"]) > 0)
    pgot1 = hg.pruneCandidates(idx[:1], 1, fixed_id=fid)
    assert pgot1["pruned"].tolist() == [0] and abs(pgot1["cond_loss"][0] - pref["cond_loss"][0]) <= tep._bounds(pref, psingle)[0][0][0]
    pgotf = hg.pruneCandidates(idx[5:6], 1, fixed_id=fid)       # the edge to the fixed vertex alone: one column
    assert pgotf["pruned"].tolist() == [0] and abs(pgotf["cond_loss"][0] - pref["rounds"][0][5][0]) <= tep._bounds(pref, psingle)[0][0][5]
    assert hip_ctx.greedy_stats()["column_vertices"] == 1
    # the 4-cycle
    for cyc, decided in ((tep._cycle_graph(), False), (tep._tie_free_cycle(), True)):
        cg = GraphWrapperHIP.from_dict(cyc, ctx=hip_ctx)
        Tc, Hc = tep._cycle_reference(cyc)
        refc = pr.greedy_sigma(np.linalg.inv(Hc), Tc, [True] * 4, 4)
        gotc = cg.pruneEdges(np.arange(4, dtype=np.int32), 4, fixed_id=0)
        assert len(gotc["pruned"]) == 1 and cg.numEdges() == 3 and hip_ctx.greedy_stats()["rounds"] == 1
        if decided:
            assert gotc["pruned"].tolist() == refc["pruned"].tolist()
            assert abs(gotc["cond_loss"][0] - refc["cond_loss"][0]) <= 1e-9 and abs(gotc["kld"][0] - refc["kld"][0]) <= 1e-9
        want = np.full(4, abi.PRUNE_BRIDGE)
        want[gotc["pruned"][0]] = abi.PRUNE_PRUNED
        assert np.array_equal(gotc["status"], want) and np.all(np.isnan(gotc["final_loss"]))
        rest = np.arange(4) != gotc["pruned"][0]
        assert np.all(np.abs(gotc["final_margin"][rest]) < 1e-8) and np.isnan(gotc["final_margin"][~rest]).all()
        again = cg.pruneCandidates(np.arange(3, dtype=np.int32), 3, fixed_id=0)
        assert len(again["pruned"]) == 0 and np.all(again["status"] == abi.PRUNE_BRIDGE)


@pytest.mark.gpu
def test_lookahead_and_cache_budget_change_cost_not_results(hip_ctx, lazy):
    """The graded prune list on the sphere fixture: lookahead 1 and 0 give the same sequence, values within the summed bounds
    of each other; a full panel has cache hits and fewer sweeps; SPG_GREEDY_CACHE_STRIPS=2 (the diagnostic cap of the
    column cache) gives the same sequence with evictions; two identical runs are bit-identical.
    Measured on an MI355X (hits / column vertices / sweeps): lookahead 1: 0 / 16 / 8, full panel: 12 / 20 / 2, two strips:
    0 / 16 / 8."""
    from tests.test_relative_covariance import _small_graphs
    case, n = tep.CASES[1]
    sub, graphs, kept = _small_graphs(case, n, hip_ctx)
    d = sub["pose_dim"]
    hg, og = graphs[0]
    ids = [int(i) for i in hg.vertices()[0]]
    fid = ids[0]
    ij, meas, info, rank, T, H1, Sig1 = tep._problem(d, hg, fid, og.information(fid))
    ref = pr.greedy_sigma(Sig1, T, [True] * tep.N_ADD, K)
    single = _single_bounds(d, T, Sig1)
    bounds, kb, _ = tep._bounds(ref, single)
    idx = tep._add_list(hg, ij, meas, info)
    runs, stats = {}, {}
    for name, look, strips in (("one", 1, None), ("full", 0, None), ("full again", 0, None), ("two strips", 0, "2")):
        os.environ.pop("SPG_GREEDY_CACHE_STRIPS", None)
        if strips:
            os.environ["SPG_GREEDY_CACHE_STRIPS"] = strips
        lazy(abi.GREEDY_LAZY, look)
        runs[name] = hg.pruneCandidates(idx, K, fixed_id=fid)
        stats[name] = hip_ctx.greedy_stats()
        assert np.array_equal(runs[name]["pruned"], ref["pruned"]), name
    os.environ.pop("SPG_GREEDY_CACHE_STRIPS", None)
    for k in runs["full"]:
        assert np.array_equal(runs["full"][k], runs["full again"][k], equal_nan=True), k
    for name in ("full", "two strips"):
        for t in range(K):
            s = int(ref["pruned"][t])
            assert abs(runs[name]["cond_loss"][t] - runs["one"]["cond_loss"][t]) <= 2 * bounds[t][s], (name, t)
            assert abs(runs[name]["kld"][t] - runs["one"]["kld"][t]) <= 2 * kb[t], (name, t)
    assert stats["one"]["column_hits"] <= stats["full"]["column_hits"] and stats["full"]["column_hits"] > 0
    assert stats["full"]["rhs_batches"] < stats["one"]["rhs_batches"] <= K
    assert stats["two strips"]["cache_bytes"] < stats["full"]["cache_bytes"]
    assert stats["two strips"]["evictions"] > 0 and stats["full"]["evictions"] == 0
    print("lazy prune, sphere: hits / vertices / sweeps", {k: (v["column_hits"], v["column_vertices"], v["rhs_batches"]) for k, v in stats.items()})
    hg.removeEdges(idx)


# One graph past the joint bound serves both twins below.
_BIG = {}


def _big_sphere(hip_ctx):
    """synth_sphere(8000, ring 80): 7 999 non-fixed SE3 vertices, 47 994 > 46 000 variables. 40 far-pair edges are added,
    graded weakest-first as tep._graded_edges grades them, from relativeCovariances (lambda_i) and the diagonal blocks of
    marginalCovariances (max|Sigma|: Sigma is PSD, its largest entry lies on the diagonal); no dense inverse."""
    if _BIG:
        return _BIG
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_sphere(n_poses=8000, ring=80)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    d = 6
    ids = [int(i) for i in hg.vertices()[0]]
    fid = ids[0]
    assert (len(ids) - 1) * d > 46000
    poses = _poses(hg)
    far = _far_pairs(hg, tep.N_ADD, seed=fid)
    rel, cov = hg.relativeCovariances(far, fixed_id=fid)
    scale = float(np.abs(hg.marginalCovariances(fixed_id=fid)[1]).max())
    base, gg, cap = tep.GRADE
    meas = np.array([rr.between(d, poses[int(a)], poses[int(b)]) for a, b in far])
    lam = np.array([np.trace(c) / d for c in cov])
    jn = np.array([np.abs(np.hstack(rr.edge(d, poses[int(a)], poses[int(b)], meas[k])[1:])).sum(axis=1).max() for k, (a, b) in enumerate(far)])
    q = lam / (jn ** 2 * scale)
    rank = np.zeros(tep.N_ADD, int)
    rank[np.argsort(-q, kind="stable")] = np.arange(tep.N_ADD)
    info = np.array([rr.upper(base * gg ** -(cap - min(int(rank[i]), cap)) / lam[i] * np.eye(d)) for i in range(tep.N_ADD)])
    _BIG.update(g=g, hg=hg, d=d, ids=ids, fid=fid, poses=poses, far=far, meas=meas, info=info, scale=scale)
    return _BIG


def _sub_terms(B, hg, ij, meas, info):
    """terms and the joint covariance over the distinct endpoints of the listed edges alone (a merged path)"""
    d, fid = B["d"], B["fid"]
    ends = sorted({int(v) for v in np.asarray(ij).ravel()} - {fid})
    Sig = hg.jointMarginalCovariance(ends, fixed_id=fid)
    T = sr.terms(d, B["poses"], {v: k for k, v in enumerate(ends)}, ij, meas, info)
    return T, Sig


@pytest.mark.gpu
def test_pruning_past_the_joint_bound(hip_ctx, lazy):
    """Every binary edge of the 8 000-pose sphere plus 40 graded far-pair edges as candidates, K = 8: JOINT raises
    SPG_ECAPACITY; LAZY and AUTO prune 8 and the stats say lazy. With S the pruned set, Sigma_S from
    jointMarginalCovariance over its endpoints and prune_ref.greedy_sigma on S alone (k = |S|): the final KLD and the sum
    of the losses, both independent of the order, agree within kb[-1]; the final KLD agrees with kullbackLeibler(original,
    pruned clone) within kb[-1] + 1e-12 |ln det|. S consists of graded edges.
    Measured on an MI355X: kld[-1] = 2.108e-8, error / bound 1.5e-11 (kld and sum of the losses); against kullbackLeibler
    1.6e-5 of what is allowed."""
    B = _big_sphere(hip_ctx)
    hg, d, fid = B["hg"], B["d"], B["fid"]
    ne = hg.numEdges()
    added = tep._add_list(hg, B["far"], B["meas"], B["info"])
    try:
        cand, eij, edata, _ = tep._binary_edges(hg)
        assert len(cand) == ne + tep.N_ADD and len(cand) > 15000
        lazy(abi.GREEDY_JOINT)
        with pytest.raises(SpgError, match="46k"):
            hg.pruneCandidates(cand, K, fixed_id=fid)
        got = {}
        for method in (abi.GREEDY_LAZY, abi.GREEDY_AUTO):
            lazy(method, 0)
            got[method] = hg.pruneCandidates(cand, K, fixed_id=fid)
            st = hip_ctx.greedy_stats()
            assert len(got[method]["pruned"]) == K and st["method"] == abi.GREEDY_LAZY and st["rounds"] == K and st["refactorised"] == 1
            assert hg.last_covariance_stats["endpoints"] == len(B["ids"]) - 1
        for k in got[abi.GREEDY_LAZY]:
            assert np.array_equal(got[abi.GREEDY_LAZY][k], got[abi.GREEDY_AUTO][k], equal_nan=True), k
        g8 = got[abi.GREEDY_LAZY]
        S = cand[g8["pruned"]]
        assert np.all(S >= ne), ("own edges were pruned: the grading, not the tolerance, is at fault", S, ne)
        ps = abi.pose_stride(d)
        sij, sdata = eij[g8["pruned"]], edata[g8["pruned"]]
        T, SigS = _sub_terms(B, hg, sij, sdata[:, :ps], sdata[:, ps:])
        ref = pr.greedy_sigma(SigS, T, [True] * K, K)
        assert len(ref["pruned"]) == K
        single = _single_bounds(d, T, SigS)     # max|Sigma| over S alone: at most the whole graph's, so no wider
        _, kb, _ = tep._bounds(ref, single)
        kerr, lerr = abs(g8["kld"][-1] - ref["kld"][-1]), abs(g8["cond_loss"].sum() - ref["cond_loss"].sum())
        print(f"lazy prune past the joint bound: kld {g8['kld'][-1]:.12g} error / bound {kerr / kb[-1]:.2e}, sum of losses error / bound {lerr / kb[-1]:.2e}")
        assert kerr <= kb[-1] and lerr <= kb[-1]
        clone = hg.clonePortion(max(B["ids"]), optimize=False)
        clone.removeEdges(S)
        kl = hg.kullbackLeibler(clone, fixed_id=fid)
        t = hg.last_kld_terms
        allowed = kb[-1] + 1e-12 * (abs(t["logdetx"]) + abs(t["logdety"]))
        print(f"lazy prune past the joint bound: kullbackLeibler {kl:.12g}, deviation / allowed {abs(g8['kld'][-1] - kl) / allowed:.2e}")
        assert abs(g8["kld"][-1] - kl) <= allowed
    finally:
        hg.removeEdges(added)


@pytest.mark.gpu
def test_selection_past_the_joint_bound(hip_ctx, lazy):
    """The selection twin: 7 900 star candidates (hub, v), which cost one column in round 0, plus the 40 graded far pairs,
    K = 8: JOINT raises SPG_ECAPACITY, LAZY and AUTO select 8; the sum of cond_gain equals select_ref on the selected set
    alone (independent of the order) within sum (t + 1) single.
    Measured on an MI355X: sum of the gains 7.365, error / allowed 6e-15."""
    B = _big_sphere(hip_ctx)
    hg, d, fid, ids = B["hg"], B["d"], B["fid"], B["ids"]
    hub = ids[len(ids) // 2]
    others = [v for v in ids if v not in (hub, fid)][:7900]
    star = np.array([(hub, v) for v in others], np.int32)
    poses = B["poses"]
    smeas = np.array([rr.between(d, poses[hub], poses[v]) for v in others])
    sinfo = np.tile(rr.upper(1e-3 * np.eye(d)), (len(others), 1))
    ij = np.ascontiguousarray(np.concatenate([star, B["far"]]), np.int32)
    meas, info = np.concatenate([smeas, B["meas"]]), np.concatenate([sinfo, B["info"]])
    assert len({int(v) for v in ij.ravel()} - {fid}) * d > 46000
    lazy(abi.GREEDY_JOINT)
    with pytest.raises(SpgError, match="46k"):
        hg.selectCandidates(ij, meas, info, K, fixed_id=fid)
    got = {}
    for method in (abi.GREEDY_LAZY, abi.GREEDY_AUTO):
        lazy(method, 0)
        got[method] = hg.selectCandidates(ij, meas, info, K, fixed_id=fid)
        st = hip_ctx.greedy_stats()
        assert len(got[method]["selected"]) == K and st["method"] == abi.GREEDY_LAZY and st["rounds"] == K
    for k in got[abi.GREEDY_LAZY]:
        assert np.array_equal(got[abi.GREEDY_LAZY][k], got[abi.GREEDY_AUTO][k], equal_nan=True), k
    g8 = got[abi.GREEDY_LAZY]
    sel = g8["selected"]
    T, SigS = _sub_terms(B, hg, ij[sel], meas[sel], info[sel])
    ref = sr.greedy_sigma(SigS, T, [True] * K, K)
    single = _single_bounds(d, T, SigS)     # max|Sigma| over S alone: at most the whole graph's, so no wider
    allowed = sum((t + 1) * single[i] for t, i in enumerate(ref["selected"]))
    err = abs(g8["cond_gain"].sum() - ref["cond_gain"].sum())
    print(f"lazy select past the joint bound: sum of gains {g8['cond_gain'].sum():.12g}, error / allowed {err / allowed:.2e}")
    assert len(ref["selected"]) == K and err <= allowed


_FACADE_SRC = r"""
#include <cstdio>
#include <numeric>
#include "spg_graph_wrapper.hpp"
int main(int argc, char **argv) {
    if (argc < 3) return 2;
    try {
        spg::GraphWrapperHIP g(argv[1]);
        g.setGreedyMethod(spg::GraphWrapperHIP::GreedyLazy, 0);
        std::vector<int> idx;
        for (int e = 0; e < g.numEdges(); e += 3) idx.push_back(e);
        auto R = g.pruneCandidates(idx, 6);
        const spg_greedy_stats st = g.greedyStats();
        FILE *f = fopen(argv[2], "w");
        for (size_t t = 0; t < R.pruned.size(); t++) fprintf(f, "%d %.17g %.17g\n", R.pruned[t], R.cond_loss[t], R.kld[t]);
        fprintf(f, "%d %d %d\n", st.method, st.rounds, st.refactorised);
        fclose(f);
        printf("lazy ok\n");
    } catch (const std::exception &e) { printf("error: %s\n", e.what()); return 1; }
    return 0;
}
"""


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_lazy_calls_leave_everything_else_untouched(d, hip_ctx, lazy):
    """After LAZY select and prune calls, scoreCandidates, pairCovariances and a JOINT select / prune on the same graph
    return what they returned before, bit for bit, and the graph is unmodified."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    from tests.test_relative_covariance import _gate_candidates, _gate_graph
    g = _gate_graph(d)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    fid = int(g["ids"][0])
    ij, meas, info, _ = _gate_candidates(d, g)
    ij, meas, info = ij[:40], meas[:40], info[:40]
    epairs = np.ascontiguousarray(g["edge_ij"][:50], np.int32)
    cand = np.arange(0, hg.numEdges(), 7, dtype=np.int32)

    def calls():
        lazy(abi.GREEDY_JOINT)
        out = dict(hg.scoreCandidates(ij, meas, info, fixed_id=fid))
        out.update({"sel_" + k: v for k, v in hg.selectCandidates(ij, meas, info, 4, fixed_id=fid).items()})
        out.update({"prn_" + k: v for k, v in hg.pruneCandidates(cand, 5, fixed_id=fid).items()})
        out["pair"] = hg.pairCovariances(epairs, fixed_id=fid)
        return out
    before, e0, v0 = calls(), hg.edges(), hg.vertices()
    lazy(abi.GREEDY_LAZY, 0)
    ls = hg.selectCandidates(ij, meas, info, 4, fixed_id=fid)
    lp = hg.pruneCandidates(cand, 5, fixed_id=fid)
    assert np.array_equal(ls["selected"], before["sel_selected"]) and np.array_equal(lp["pruned"], before["prn_pruned"])
    assert np.allclose(ls["cond_gain"], before["sel_cond_gain"], rtol=1e-6, atol=0) and np.allclose(lp["kld"], before["prn_kld"], rtol=1e-6, atol=1e-12)
    after, e1, v1 = calls(), hg.edges(), hg.vertices()
    for k in e0:
        assert np.array_equal(e0[k], e1[k]), k
    assert np.array_equal(v0[0], v1[0]) and np.array_equal(v0[1], v1[1])
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k


@pytest.mark.gpu
def test_cpp_facade_lazy_pruning_matches_python(tmp_path, hip_ctx, lazy):
    """setGreedyMethod / greedyStats of the C++ façade: a lazy pruning of every third edge of a small sphere equals the
    Python binding's, bit for bit."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_sphere(n_poses=200, ring=20)
    path = str(tmp_path / "s200.g2o")
    g2o_io.write_g2o(path, g)
    src, exe = str(tmp_path / "lazy_facade.cpp"), str(tmp_path / "lazy_facade")
    open(src, "w").write(_FACADE_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, src, "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, path, str(tmp_path / "cpp.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and "lazy ok" in out.stdout, out.stdout + out.stderr
    rows = [ln.split() for ln in open(str(tmp_path / "cpp.txt")).read().splitlines()]
    cpp = np.array([[float(x) for x in r] for r in rows[:-1]])
    assert [int(x) for x in rows[-1]] == [abi.GREEDY_LAZY, 6, 1]
    hg = GraphWrapperHIP.load(path, ctx=hip_ctx)
    lazy(abi.GREEDY_LAZY, 0)
    got = hg.pruneCandidates(np.arange(0, hg.numEdges(), 3, dtype=np.int32), 6)
    assert len(cpp) == 6 and np.array_equal(cpp[:, 0].astype(np.int32), got["pruned"])
    assert np.array_equal(cpp[:, 1], got["cond_loss"]) and np.array_equal(cpp[:, 2], got["kld"])
