"""Greedy selection of loop-closure candidates by conditional information gain (spg_graph_select_candidates,
csrc/spg_sparse.inc: sp_select_init_kernel / _argmax_kernel / _pick_kernel / _round_kernel) against the numpy rule of
tests/select_ref.py.
CPU: the candidate-space recurrence equals the rule on the dense information (slogdet), the GPU fixtures are decidable,
the argument contract on an injected backend, the ABI and the bindings, the C++ demo compiles.
GPU: sequence and gains on small graphs (before and after marginalisation, both gauges), the log det identity through
information() and addEdge, the reduction over several workgroups and the stop rules, untouched behaviour, the C++ façade.

Bounds (derived, not measured). A single gain is held to the bound of tests/test_relative_covariance.py:
single_i = 1/2 D ||Omega_i||2 D beta_i, beta_i = ||J_i||inf^2 1e-9 max|Sigma| + 1e-11 max|C_ii(0)| with the reference's
C_ii(0) and Sigma. A gain read after t conditionings (cond_gain[t]; final_gain after the last round) is held to
(t + 1) single_i: each conditioning subtracts B B^T = C_i* L* M^-1 L*^T C_*i, a term of the same form as C_ii and below it
in the PSD order (M >= I keeps ||L* G^-T|| <= ||L*||), so it adds at most one more error term of the size of the first.
The fixtures are decidable when in every round the best candidate leads the best distinct other candidate (identical copies
of one record excluded) by at least 10 times the larger of their two bounds.
Measured on an MI355X, worst error over its bound: cond_gain / final_gain 3.5e-6 (intel), 1.6e-7 (sphere), 4.7e-6
(manhattan GLC Tree), 2.7e-10 (synth_manhattan, 300 candidates); the sum of the gains against 1/2 delta ln det of
information(): 1.7e-7, 1.7e-8 and 4.7e-7 of what is allowed. Smallest lead over 10 bounds (numpy alone): intel 128,
sphere 6.3, manhattan GLC Tree 55, synth_manhattan 2.1.
The three small cases reach their lead with graded isotropic informations (GRADE, _graded_info): at the scale of the
graphs' own edges the single-gain bound exceeds the spacing of the gains (sphere: 1 to 16 nats against gains of 5 to 9).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sparsifyposegraph_amd import abi, g2o_io, lib
from sparsifyposegraph_amd.lib import SpgError
from tests import oracle_lib, util
from tests import relative_ref as rr
from tests import select_ref as sr
from tests.test_covariance_blocks import _edge_pairs, _non_adjacent_pair, _oracle_of, _small
from tests.test_relative_covariance import CHI2_99, _far_pairs, _gate_candidates, _gate_graph, _perturbed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")
_f64p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
EINVAL, ESTATE = -1, -7
CASES = [("intel_nfr_tree_sp3", 600), ("sphere_nfr_tree", 500), ("manhattan_glc_tree", 600)]
# Omega of the candidates. At the scale of the graphs' own edges the bounds above (which carry ||Omega||2 ||J||inf^2
# max|Sigma|) exceed the spacing of the gains (on the sphere: 1 to 16 nats against gains of 5 to 9, a lead of 5.8e-6), and
# scaling Omega alone does not reach 10 bounds there (8.5e-2 at best). The lists are therefore built to be decidable:
# GRADE = (base, g), isotropic informations graded by _graded_info, the leader's Omega P of size base and each further rank
# g times weaker, the candidates with the tightest bounds ranked first.
GRADE = (1.0, 2.0)
K = 8
I_COPY, I_FIXED_A, I_FIXED_B, I_BAD, N_CAND = 55, 58, 59, 60, 61


# ------------------------------------------------------------------------------------------------- shared helpers
def _poses(view):
    ids, poses = view.vertices()
    return {int(i): np.array(p) for i, p in zip(ids, poses)}


def _at(ids, fid):
    return {v: k for k, v in enumerate(int(i) for i in ids if int(i) != fid)}


def _single_bounds(d, T, Sig):
    """single_i of the module docstring per candidate (NaN where Omega is unusable), from the reference's own numbers"""
    scale = float(np.abs(Sig).max())
    out = np.full(len(T), np.nan)
    for i, t in enumerate(T):
        if not t["ok"]:
            continue
        idx, J = sr._support(t, d)
        P = J @ Sig[np.ix_(idx, idx)] @ J.T
        beta = np.abs(t["J"]).sum(axis=1).max() ** 2 * 1e-9 * scale + 1e-11 * np.abs(P).max()
        out[i] = 0.5 * d * np.linalg.norm(t["Om"], 2) * d * beta
    return out


def _lead(ref, single, same=()):
    """smallest (best - best distinct other) / (10 * bound of the round) over the rounds of a reference run"""
    worst = np.inf
    for t, g in enumerate(ref["rounds"][:len(ref["selected"])]):
        best = int(ref["selected"][t])
        others = [i for i in g if i != best and not (best in same and i in same)]
        if not others:
            continue
        second = max(others, key=lambda i: g[i])
        worst = min(worst, (g[best] - g[second]) / (10.0 * (t + 1) * max(single[best], single[second])))
    return worst


def _graded_info(d, T, Sig, copy, base, g):
    """Isotropic informations s_i I that space the gains by design. With lambda_i = tr(C_ii(0)) / D on the reference's
    covariance, s_i = base g^-rank_i / lambda_i: the ranks follow the descending order of q_i = lambda_i / (||J_i||inf^2
    max|Sigma|), the ratio of a candidate's gain to its bound, so the candidates whose bound is tight lead and the leader's
    Omega P is of size `base` (not the weak-information regime); candidate `copy` (the one listed three times) is moved to
    rank K - 1, so that its lowest copy is the last of the K choices and the two others stay eligible. Ranks stop at 20."""
    scale = float(np.abs(Sig).max())
    lam, q = np.zeros(len(T)), np.zeros(len(T))
    for i, t in enumerate(T):
        idx, J = sr._support(t, d)
        lam[i] = np.trace(J @ Sig[np.ix_(idx, idx)] @ J.T) / d
        q[i] = lam[i] / (np.abs(t["J"]).sum(axis=1).max() ** 2 * scale)
    last = len(T) - 1                                   # the candidate whose Omega is made indefinite: never eligible
    order = [int(i) for i in np.argsort(-q, kind="stable") if i not in (copy, last)]
    order.insert(K - 1, copy)
    order.append(last)
    rank = np.zeros(len(T))
    rank[order] = np.minimum(np.arange(len(T)), 20)
    return np.array([rr.upper(base * g ** -rank[i] / lam[i] * np.eye(d)) for i in range(len(T))]), q


def _small_candidates(d, view, sub, fid, Sig, grade):
    """The 61 candidates of the sequence test on a graph view (vertices(), edges()): 40 far pairs, 10 edge pairs, 5 pairs
    sharing one endpoint, one far pair three times with identical records (the far pair, of 41 drawn, with the tightest
    bound), the fixed vertex as a and as b, and one candidate with an indefinite Omega. Omega: the graded isotropic
    informations of _graded_info with grade = (base, g), the tripled pair ranked last of the K choices; z = the current
    relative pose composed with 0 to 4 sigma of a random edge of the input graph. Returns (ij, meas, info)."""
    ids = [int(i) for i in view.vertices()[0]]
    poses = _poses(view)
    ps = abi.pose_stride(d)
    rng = np.random.default_rng(1000 + fid)
    far = _far_pairs(view, 41, seed=fid)
    ep = _edge_pairs(view)
    edge = ep[:: max(1, len(ep) // 10)][:10]
    hub = ids[len(ids) // 3]
    share = np.array([(hub, v) for v in rng.choice([v for v in ids if v != hub], size=5, replace=False)], np.int32)
    other = [v for v in ids if v != fid]
    fixed = np.array([(fid, other[len(other) // 2]), (other[-1], fid)], np.int32)
    pairs = np.concatenate([far, edge, share, fixed, far[:1]])
    info = sub["edge_data"][rng.integers(len(sub["edge_data"]), size=len(pairs)), ps:]
    meas = np.array([_perturbed(d, rr.between(d, poses[int(a)], poses[int(b)]), rr.omega(d, info[k]), 4.0 * rng.random(), rng)
                     for k, (a, b) in enumerate(pairs)])     # sigma: that of a random edge's information
    T = sr.terms(d, poses, _at(ids, fid), pairs, meas, info)
    _, q = _graded_info(d, T, Sig, 0, *grade)
    top = int(np.argmax(q[:41]))
    info, _ = _graded_info(d, T, Sig, top, *grade)
    w, V = np.linalg.eigh(rr.omega(d, info[-1]))
    w[0] = -0.5 * w[1]
    info[-1] = rr.upper(V @ np.diag(w) @ V.T)
    keep = [i for i in range(41) if i != top]
    order = keep + list(range(41, 56)) + [top] * 3 + [56, 57, 58]
    assert len(order) == N_CAND and order[I_COPY] == top and order[I_BAD] == 58
    return np.ascontiguousarray(pairs[order], np.int32), meas[order], info[order]


def _reference(d, view, fid, Sig, ij, meas, info, k, min_gain=0.0, eligible=None):
    ids = [int(i) for i in view.vertices()[0]]
    T = sr.terms(d, _poses(view), _at(ids, fid), ij, meas, info)
    elig = [t["ok"] for t in T] if eligible is None else [t["ok"] and bool(e) for t, e in zip(T, eligible)]
    ref = sr.greedy_sigma(Sig, T, elig, k, min_gain)
    return ref, _single_bounds(d, T, Sig), T


def _fids(ids, kept):
    return ids[0], kept[len(kept) // 2]


# ------------------------------------------------------------------------------------------------------- CPU
def _random_problem(d, seed, n_cand=12):
    rng = np.random.default_rng(seed)
    nv = 8
    A = rng.normal(size=(nv * d, nv * d))
    H = A @ A.T + nv * d * np.eye(nv * d)
    poses = {v: (rng.normal(size=3) if d == 3 else np.concatenate([rng.normal(size=3), q / np.linalg.norm(q)]))
             for v, q in zip(range(nv + 1), rng.normal(size=(nv + 1, 4)))}
    at = {v: v for v in range(nv)}      # vertex nv is the fixed one
    ij = np.array([rng.choice(nv + 1, size=2, replace=False) for _ in range(n_cand)], np.int32)
    ij[0] = (nv, 3)
    info = np.array([rr.upper(B @ B.T + np.eye(d)) for B in rng.normal(size=(n_cand, d, d))])
    meas = np.array([rr.compose(d, rr.between(d, poses[int(a)], poses[int(b)]), rr.from_mqt(0.05 * rng.normal(size=6)) if d == 6
                                else 0.05 * rng.normal(size=3)) for a, b in ij])
    return H, sr.terms(d, poses, at, ij, meas, info)


@pytest.mark.parametrize("d", [3, 6])
def test_recurrence_equals_the_rule_on_the_dense_information(d):
    """Random SPD H over 8 poses, 12 candidates (one with the fixed vertex), k = 6: the candidate-space recurrence and the
    Woodbury form on the dense covariance give the sequence of the slogdet rule and its gains to 1e-10 (relative); the
    conditional gain of a fixed candidate never increases; the sum of the gains is 1/2 (ln det H_final - ln det H)."""
    H, T = _random_problem(d, seed=d)
    elig = [True] * len(T)
    exact = sr.greedy(H, T, elig, 6)
    Sig = np.linalg.inv(H)
    for other in (sr.recurrence(Sig, T, elig, 6), sr.greedy_sigma(Sig, T, elig, 6)):
        assert np.array_equal(other["selected"], exact["selected"]) and len(exact["selected"]) == 6
        assert np.allclose(other["cond_gain"], exact["cond_gain"], rtol=1e-10, atol=0)
        live = ~np.isnan(exact["final_gain"])
        assert np.array_equal(live, ~np.isnan(other["final_gain"])) and live.sum() == 6
        assert np.allclose(other["final_gain"][live], exact["final_gain"][live], rtol=1e-10, atol=0)
        for t in range(1, len(other["rounds"])):
            for i, g in other["rounds"][t].items():
                assert g <= other["rounds"][t - 1][i] * (1 + 1e-12)
    want = 0.5 * (np.linalg.slogdet(exact["H"])[1] - np.linalg.slogdet(H)[1])
    assert exact["cond_gain"].sum() == pytest.approx(want, rel=1e-12)
    # min_gain between the third and the fourth gain stops after three
    mid = 0.5 * (exact["cond_gain"][2] + exact["cond_gain"][3])
    assert np.array_equal(sr.recurrence(Sig, T, elig, 6, mid)["selected"], exact["selected"][:3])


@pytest.mark.parametrize("d", [3, 6])
def test_second_of_two_identical_candidates(d):
    """The same candidate twice: the first copy is chosen, and the second's conditional gain is
    1/2 ln det(I + Omega (P^-1 + Omega)^-1), P the covariance of its error before the first was added."""
    H, T = _random_problem(d, seed=10 + d, n_cand=3)
    T = [T[1], T[1]]
    Sig = np.linalg.inv(H)
    got = sr.recurrence(Sig, T, [True, True], 2)
    assert got["selected"].tolist() == [0, 1]
    idx, J = sr._support(T[0], d)
    P, Om = J @ Sig[np.ix_(idx, idx)] @ J.T, T[0]["Om"]
    want = 0.5 * np.linalg.slogdet(np.eye(d) + Om @ np.linalg.inv(np.linalg.inv(P) + Om))[1]
    assert got["cond_gain"][1] == pytest.approx(want, rel=1e-10)
    assert got["cond_gain"][1] < got["cond_gain"][0]


def _oracle_graphs(case, n):
    """The oracle twins of _small_graphs on the CPU: (sub, (before, after), kept ids)"""
    g, which, opts, *_ = util.load_golden(case)
    sub, w = util.prefix_graph(g, which, n)
    base, sp = oracle_lib.OracleGraph.from_dict(sub), oracle_lib.OracleGraph.from_dict(sub)
    assert sp.marginalize(w, opts) == 0
    return sub, (base, sp), [int(i) for i in sp.vertices()[0]]


@pytest.mark.parametrize("case,n", CASES)
def test_small_fixtures_are_decidable(case, n):
    """A condition on the inputs of the GPU sequence test: on the oracle's graphs (before and after its own marginalisation,
    both gauges) every round's lead is at least 10 bounds and the copies of the tripled candidate are chosen in ascending
    index order: exactly the lowest copy is chosen, in the last round, and the two others stay eligible. On a sub-list of every case (after the marginalisation, first
    gauge: the first five choices, a second copy and two more, k = 3) the slogdet rule itself gives the Woodbury form's
    sequence and gains."""
    sub, graphs, kept = _oracle_graphs(case, n)
    d = sub["pose_dim"]
    worst, checked_exact = np.inf, False
    for og in graphs:
        ids = [int(i) for i in og.vertices()[0]]
        for fid in _fids(ids, kept):
            H = og.information(fid)
            Sig = np.linalg.inv(H)
            ij, meas, info = _small_candidates(d, og, sub, fid, Sig, GRADE)
            ref, single, T = _reference(d, og, fid, Sig, ij, meas, info, K)
            same = (I_COPY, I_COPY + 1, I_COPY + 2)
            worst = min(worst, _lead(ref, single, same))
            assert len(ref["selected"]) == K and I_BAD not in ref["selected"]
            copies = [i for i in ref["selected"] if i in same]
            assert copies == list(same[:len(copies)]) and copies == [I_COPY]
            assert ref["selected"][-1] == I_COPY and np.all(np.isfinite(ref["final_gain"][[I_COPY + 1, I_COPY + 2]]))
            if og is graphs[1] and not checked_exact:
                few = list(dict.fromkeys([int(i) for i in ref["selected"][:5]] + [I_COPY, I_COPY + 1, 0, 1]))
                Tf = [T[i] for i in few]
                exact = sr.greedy(H, Tf, [True] * len(few), 3)
                fast = sr.greedy_sigma(Sig, Tf, [True] * len(few), 3)
                atol = 1e-12 * abs(np.linalg.slogdet(H)[1])      # a gain of the slogdet rule is a difference of two ln det
                assert np.array_equal(exact["selected"], fast["selected"]) and len(exact["selected"]) == 3
                assert np.allclose(exact["cond_gain"], fast["cond_gain"], rtol=1e-9, atol=atol)
                live = ~np.isnan(exact["final_gain"])
                assert np.allclose(exact["final_gain"][live], fast["final_gain"][live], rtol=1e-9, atol=atol)
                checked_exact = True
    print(f"{case}[{n}]: smallest lead / (10 bounds) {worst:.2e}")
    assert checked_exact and worst >= 1.0


def _manhattan_candidates(g, view):
    """300 candidates on synth_manhattan(400): random far pairs, Omega of the generator, z = the current relative pose
    composed with 0 to 4 sigma; candidate 7 has an indefinite Omega."""
    d = 3
    rng = np.random.default_rng(77)
    poses = _poses(view)
    ij = _far_pairs(view, 300, seed=78)
    info = np.tile(g["edge_data"][0, 3:], (300, 1))
    meas = np.array([_perturbed(d, rr.between(d, poses[int(a)], poses[int(b)]), rr.omega(d, info[k]), 4.0 * rng.random(), rng)
                     for k, (a, b) in enumerate(ij)])
    info[7] = rr.upper(np.diag([1.0, -1.0, 1.0]))
    return ij, meas, info


def test_manhattan_fixture_is_decidable():
    g = g2o_io.synth_manhattan(n_poses=400, side=20)
    og = oracle_lib.OracleGraph.from_dict(g)
    fid = int(g["ids"][0])
    ij, meas, info = _manhattan_candidates(g, og)
    ref, single, _ = _reference(3, og, fid, np.linalg.inv(og.information(fid)), ij, meas, info, 5)
    lead = _lead(ref, single)
    print(f"synth_manhattan(400), 300 candidates: smallest lead / (10 bounds) {lead:.2e}")
    assert len(ref["selected"]) == 5 and lead >= 1.0
    # the stop rule of the GPU test: the midpoint between the third and the fourth gain is 10 bounds from both
    mid = 0.5 * (ref["cond_gain"][2] + ref["cond_gain"][3])
    assert min(ref["cond_gain"][2] - mid, mid - ref["cond_gain"][3]) >= 10 * 4 * max(single[ref["selected"][2]], single[ref["selected"][3]])


def test_abi_and_bindings_cover_the_selection():
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    assert "spg_graph_select_candidates" in lib.SYMBOLS
    assert hasattr(C.CDLL(lib.LIB_PATH), "spg_graph_select_candidates")
    assert (abi.CAND_SCORED, abi.CAND_INFO_NOT_PD, abi.CAND_GATED, abi.CAND_SELECTED) == (0, 1, 2, 3)
    assert C.sizeof(abi.SelectStats) == C.sizeof(abi.CovSolveStats) + 16
    assert set(abi.SelectStats().asdict()) >= {"rounds", "endpoints", "select_seconds", "solve_seconds", "device_seconds", "columns"}
    assert callable(GraphWrapperHIP.selectCandidates)
    hdr = open(os.path.join(ROOT, "include", "spg.h")).read()
    assert "SPG_CAND_GATED = 2" in hdr and "SPG_CAND_SELECTED = 3" in hdr and "NOT re-evaluated" in hdr


def test_select_checks_arguments_before_the_backend():
    """On an injected (CPU) context: the size queries answer; k = 0 and n = 0 return 0; an unknown id, a == b, an unknown
    fixed vertex, a non-finite measurement, k < 0 and an active stepwise marginalisation are SPG_EINVAL with their word;
    a call that would compute is SPG_ESTATE (no CPU fallback); the Python layer raises."""
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
    sel, cg, fg, status = np.zeros(n, np.int32), np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
    f = lambda x: x.ctypes.data_as(_f64p)  # noqa: E731
    i = lambda x: x.ctypes.data_as(_i32p)  # noqa: E731
    err = lambda: L.spg_last_error(ictx.h).decode()  # noqa: E731

    def select(ij, r, cnt, k, cap, fid=-1, h=a.h):
        return L.spg_graph_select_candidates(h, fid, i(ij), f(r), cnt, k, 0.0, 0.0, i(sel), f(cg), cap, f(fg), i(status), None)
    # size queries, k = 0, n = 0
    assert select(pairs, rec, n, 2, 0) == 2 and select(pairs, rec, n, 2, 1) == 2 and select(pairs, rec, n, 9, 0) == n
    assert L.spg_graph_select_candidates(a.h, -1, i(pairs), f(rec), n, 3, 0.0, 0.0, None, None, 99, None, None, None) == 3
    assert select(pairs, rec, n, 0, n) == 0 and select(pairs, rec, 0, 3, n) == 0
    # no HIP backend
    st = abi.SelectStats()
    assert select(pairs, rec, n, 2, 2) == ESTATE and "HIP backend" in err()
    assert L.spg_graph_select_candidates(a.h, -1, i(pairs), f(rec), n, n, 0.0, 0.0, i(sel), f(cg), n, None, None, C.byref(st)) == ESTATE
    # invalid arguments, answered before the backend
    unknown = np.array([int(ids[0]), 999999], np.int32)
    same = np.array([e0[0], e0[0]], np.int32)
    for bad, word in ((unknown, "999999"), (same, "same")):
        assert select(bad, rec, 1, 1, 1) == EINVAL and word in err() and "pair 0" in err()
    assert select(pairs, rec, n, 2, 2, fid=999999) == EINVAL and "fixed vertex" in err()
    assert select(pairs, rec, n, -1, 2) == EINVAL and "negative" in err()
    for bad_value in (np.nan, np.inf):
        r2 = rec.copy()
        r2[2, 1] = bad_value
        assert select(pairs, r2, n, 2, 2) == EINVAL
        assert "pair 2" in err() and f"({na[0]}, {na[1]})" in err() and "finite" in err()
    r2 = rec.copy()
    r2[1, D:] = np.nan          # a non-finite information is a status of the candidate, not an argument error
    assert select(pairs, r2, n, 2, 0) == 2
    assert L.spg_graph_select_candidates(a.h, -1, i(pairs), None, n, 2, 0.0, 0.0, i(sel), f(cg), 2, None, None, None) == EINVAL
    # an active stepwise marginalisation
    g, which, opts, *_ = util.load_golden("intel_nfr_tree_sp3")
    sub2, w = util.prefix_graph(g, which, 30)
    b = GraphWrapperHIP.from_dict(sub2, ctx=ictx)
    b.begin(w, opts, 0, 1)
    assert select(pairs, rec, n, 2, 2, h=b.h) == EINVAL and "active" in err()
    # the Python layer
    with pytest.raises(SpgError, match="HIP backend"):
        a.selectCandidates(pairs, rec[:, :D], rec[:, D:], 2)
    with pytest.raises(SpgError, match="same"):
        a.selectCandidates([same], rec[:1, :D], rec[:1, D:], 1)
    with pytest.raises(SpgError, match="negative"):
        a.selectCandidates(pairs, rec[:, :D], rec[:, D:], -1)
    with pytest.raises(ValueError):
        a.selectCandidates(pairs, rec[:, :D], rec[:, D:-1], 2)
    got = a.selectCandidates(pairs, rec[:, :D], rec[:, D:], 0)
    assert len(got["selected"]) == 0 and len(got["cond_gain"]) == 0 and got["final_gain"].shape == (n,)
    got = a.selectCandidates(np.zeros((0, 2), np.int32), np.zeros((0, D)), np.zeros((0, D * (D + 1) // 2)), 3)      # n = 0
    assert len(got["selected"]) == 0 and got["final_gain"].shape == (0,) and got["status"].shape == (0,)


def _build_demo(tmp_path):
    exe = str(tmp_path / "select_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "select_demo.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_select_demo_compiles(tmp_path):
    out = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr


# ------------------------------------------------------------------------------------------------------- GPU
def _check_against(ref, single, got, n, what):
    """selected, cond_gain and final_gain of a device run against a reference run; returns the worst error / bound"""
    r = len(ref["selected"])
    assert np.array_equal(got["selected"], ref["selected"]), (what, got["selected"], ref["selected"])
    worst = 0.0
    for t in range(r):
        err, tol = abs(got["cond_gain"][t] - ref["cond_gain"][t]), (t + 1) * single[ref["selected"][t]]
        worst = max(worst, err / tol)
        print(f"{what}: round {t} candidate {ref['selected'][t]} gain {got['cond_gain'][t]:.12g} error / bound {err / tol:.2e}")
        assert err <= tol, (what, t, err, tol)
    live = ~np.isnan(ref["final_gain"])
    assert np.array_equal(live, ~np.isnan(got["final_gain"])), what
    err = np.abs(got["final_gain"][live] - ref["final_gain"][live]) / ((r + 1) * single[live])
    if live.any():
        print(f"{what}: final gains, worst error / bound {err.max():.2e}")
        worst = max(worst, float(err.max()))
        assert err.max() <= 1.0, (what, int(np.flatnonzero(live)[err.argmax()]), err.max())
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", CASES)
def test_sequence_and_gains_on_small_graphs(case, n, hip_ctx):
    """61 candidates (_small_candidates), k = 8, before and after the case's marginalisation, both gauges: the sequence of
    the reference exactly, cond_gain[t] and final_gain within (t + 1) single bounds, the indefinite candidate reported and
    never chosen, of the three identical copies the lowest index chosen and the two others' final gains bit-identical."""
    from tests.test_relative_covariance import _small_graphs
    sub, graphs, kept = _small_graphs(case, n, hip_ctx)
    d = sub["pose_dim"]
    worst, lead = 0.0, np.inf
    for hg, og in graphs:
        ids = [int(i) for i in hg.vertices()[0]]
        for fid in _fids(ids, kept):
            Sig = np.linalg.inv(og.information(fid))
            ij, meas, info = _small_candidates(d, hg, sub, fid, Sig, GRADE)
            ref, single, _ = _reference(d, hg, fid, Sig, ij, meas, info, K)
            same = (I_COPY, I_COPY + 1, I_COPY + 2)
            lead = min(lead, _lead(ref, single, same))
            got = hg.selectCandidates(ij, meas, info, K, fixed_id=fid)
            what = f"{case}[{n}] {'after' if hg is graphs[1][0] else 'before'} fixed {fid}"
            worst = max(worst, _check_against(ref, single, got, N_CAND, what))
            want = np.zeros(N_CAND, np.int32)
            want[ref["selected"]] = abi.CAND_SELECTED
            want[I_BAD] = abi.CAND_INFO_NOT_PD
            assert np.array_equal(got["status"], want)
            copies = [i for i in got["selected"] if i in same]
            assert copies == list(same[:len(copies)])
            left = [i for i in same if i not in copies]
            assert len(left) == 2      # the lowest copy was chosen, the two others keep the same bits
            assert np.isfinite(got["final_gain"][left[0]]) and got["final_gain"][left[0]] == got["final_gain"][left[1]]
            s = hg.last_covariance_stats
            assert s["rounds"] == K and 0 < s["select_seconds"] < s["device_seconds"]
            assert s["endpoints"] == len({int(v) for v in ij.ravel()} - {fid})
    print(f"{case}[{n}]: worst error / bound {worst:.2e}, smallest lead / (10 bounds) {lead:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", CASES)
def test_selected_gains_sum_to_half_the_log_det_increase(case, n, hip_ctx):
    """Independent of select_ref: the sum of cond_gain equals 1/2 (ln det information() after addEdge of the selected
    candidates on a clone - ln det information() before), within the summed bounds plus 1e-12 |ln det|."""
    from tests.test_relative_covariance import _small_graphs
    sub, graphs, kept = _small_graphs(case, n, hip_ctx)
    d = sub["pose_dim"]
    worst = 0.0
    for hg, og in graphs:
        ids = [int(i) for i in hg.vertices()[0]]
        for fid in _fids(ids, kept):
            H0 = hg.information(fid)
            Sig = np.linalg.inv(H0)
            ij, meas, info = _small_candidates(d, hg, sub, fid, Sig, GRADE)
            got = hg.selectCandidates(ij, meas, info, K, fixed_id=fid)
            T = sr.terms(d, _poses(hg), _at(ids, fid), ij, meas, info)
            single = _single_bounds(d, T, Sig)
            clone = hg.clonePortion(max(ids), optimize=False)
            assert clone.numEdges() == hg.numEdges() and clone.numVertices() == hg.numVertices()
            for i in got["selected"]:
                clone.addEdge(int(ij[i][0]), int(ij[i][1]), meas[i], info[i])
            ld0, ld1 = np.linalg.slogdet(H0)[1], np.linalg.slogdet(clone.information(fid))[1]
            want = 0.5 * (ld1 - ld0)
            allowed = sum((t + 1) * single[i] for t, i in enumerate(got["selected"])) + 1e-12 * (abs(ld0) + abs(ld1))
            err = abs(got["cond_gain"].sum() - want)
            worst = max(worst, err / allowed)
            assert len(got["selected"]) == K and want > 0 and err <= allowed, (case, fid, got["cond_gain"].sum(), want, allowed)
    print(f"{case}[{n}]: sum of the gains against 1/2 delta ln det information(): worst deviation / allowed {worst:.2e}")


@pytest.mark.gpu
def test_reduction_over_workgroups_and_stop_rules(hip_ctx):
    """synth_manhattan(400), 300 candidates (two workgroups of argmax partials), k = 5: the reference's sequence; min_gain
    between its third and fourth gain selects exactly three; k > n selects every eligible candidate; n = 1, k = 1; with
    max_d2 at the 99 % chi^2 value on the optimised graph only inliers are selected and every outlier is gated."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_manhattan(n_poses=400, side=20)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    fid = int(g["ids"][0])
    H = np.linalg.inv(_oracle_of(hg).information(fid))      # the covariance the reference runs on
    ij, meas, info = _manhattan_candidates(g, hg)
    ref, single, _ = _reference(3, hg, fid, H, ij, meas, info, 5)
    got = hg.selectCandidates(ij, meas, info, 5, fixed_id=fid)
    _check_against(ref, single, got, 300, "manhattan 300")
    assert got["status"][7] == abi.CAND_INFO_NOT_PD and np.isnan(got["final_gain"][7])
    # min_gain
    mid = 0.5 * (ref["cond_gain"][2] + ref["cond_gain"][3])
    ref3, _, _ = _reference(3, hg, fid, H, ij, meas, info, 5, min_gain=mid)
    got3 = hg.selectCandidates(ij, meas, info, 5, min_gain=mid, fixed_id=fid)
    assert len(got3["selected"]) == 3 and hg.last_covariance_stats["rounds"] == 3
    _check_against(ref3, single, got3, 300, "manhattan 300, min_gain")
    assert (got3["status"] == abi.CAND_SELECTED).sum() == 3
    # k > n: every eligible candidate, in the reference's order; then nothing is left
    few = [5, 6, 7, 8, 9]
    refk, _, _ = _reference(3, hg, fid, H, ij[few], meas[few], info[few], 9)
    gotk = hg.selectCandidates(ij[few], meas[few], info[few], 9, fixed_id=fid)
    assert len(gotk["selected"]) == 4 and np.array_equal(gotk["selected"], refk["selected"])
    assert np.array_equal(gotk["status"], [3, 3, 1, 3, 3]) and np.all(np.isnan(gotk["final_gain"]))
    # n = 1, k = 1
    got1 = hg.selectCandidates(ij[:1], meas[:1], info[:1], 1, fixed_id=fid)
    assert got1["selected"].tolist() == [0] and abs(got1["cond_gain"][0] - ref["rounds"][0][0]) <= single[0]
    # the gate, on the optimised graph with the inliers and outliers of the scoring test
    hg.optimize(50, fixed_id=fid)
    gij, gmeas, ginfo, inlier = _gate_candidates(3, g)
    d2 = hg.scoreCandidates(gij, gmeas, ginfo, fixed_id=fid)["d2"]
    gated = hg.selectCandidates(gij, gmeas, ginfo, 10, max_d2=CHI2_99[3], fixed_id=fid)
    assert len(gated["selected"]) == 10 and np.all(inlier[gated["selected"]])
    assert np.all(gated["status"][~inlier] == abi.CAND_GATED) and np.all(np.isnan(gated["final_gain"][~inlier]))
    assert np.array_equal(gated["status"] == abi.CAND_GATED, d2 > CHI2_99[3])


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_selection_leaves_the_graph_and_the_scores_untouched(d, hip_ctx):
    """After selectCandidates the edges, the estimates and scoreCandidates' outputs are bit-identical to before; the
    round-0 gains (k = 1: cond_gain of the choice, final_gain of the rest) agree with scoreCandidates' gain within the
    single-gain bound (not bit for bit: the joint block solves a different set of columns)."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = _gate_graph(d)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)
    fid = int(g["ids"][0])
    ij, meas, info, _ = _gate_candidates(d, g)
    ij, meas, info = ij[:40], meas[:40], info[:40]
    before = hg.scoreCandidates(ij, meas, info, fixed_id=fid)
    e0, v0 = hg.edges(), hg.vertices()
    got = hg.selectCandidates(ij, meas, info, 1, fixed_id=fid)
    after = hg.scoreCandidates(ij, meas, info, fixed_id=fid)
    e1, v1 = hg.edges(), hg.vertices()
    for k in e0:
        assert np.array_equal(e0[k], e1[k]), k
    assert np.array_equal(v0[0], v1[0]) and np.array_equal(v0[1], v1[1])
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    ids = [int(i) for i in hg.vertices()[0]]
    Sig = np.linalg.inv(_oracle_of(hg).information(fid))
    single = _single_bounds(d, sr.terms(d, _poses(hg), _at(ids, fid), ij, meas, info), Sig)
    s = int(got["selected"][0])
    assert before["gain"][s] >= before["gain"].max() - single[s] and abs(got["cond_gain"][0] - before["gain"][s]) <= single[s]
    # one conditioning has been applied to the others: their gains can only have dropped
    rest = np.arange(40) != s
    assert np.all(got["final_gain"][rest] <= before["gain"][rest] + single[rest])
    none = hg.selectCandidates(ij, meas, info, 1, min_gain=1e9, fixed_id=fid)
    assert len(none["selected"]) == 0 and np.all(np.abs(none["final_gain"] - before["gain"]) <= single)


@pytest.mark.gpu
def test_cpp_facade_selection_matches_python(tmp_path, hip_ctx):
    """tests/cpp/select_demo.cpp selects 6 candidates through the façade on a small sphere and adds them; the indices and
    gains equal the Python binding's bit for bit."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_sphere(n_poses=200, ring=20)
    path = str(tmp_path / "s200.g2o")
    g2o_io.write_g2o(path, g)
    out = subprocess.run([_build_demo(tmp_path), path, "6", str(tmp_path / "cpp.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and "selection ok" in out.stdout, out.stdout + out.stderr
    cpp = np.loadtxt(str(tmp_path / "cpp.txt")).reshape(-1, 2)
    hg = GraphWrapperHIP.load(path, ctx=hip_ctx)
    ids = [int(i) for i in hg.vertices()[0]]
    n = len(ids)
    pairs = np.array([(ids[i], ids[n - 1 - i]) for i in range(n // 2)], np.int32)
    rel, _ = hg.relativeCovariances(pairs)
    e = hg.edges()
    k = next(k for k in range(len(e["kind"])) if ids[0] in e["vert_ids"][e["vert_off"][k]:e["vert_off"][k + 1]])
    info = e["data"][e["data_off"][k] + 7:e["data_off"][k + 1]]
    ij = np.concatenate([pairs, pairs[:5]])
    meas = np.concatenate([np.roll(rel, -1, axis=0), np.roll(rel, -1, axis=0)[:5]])
    got = hg.selectCandidates(ij, meas, np.tile(info, (len(ij), 1)), 6)
    assert len(cpp) == 6 and np.array_equal(cpp[:, 0].astype(np.int32), got["selected"]) and np.array_equal(cpp[:, 1], got["cond_gain"])
