"""Joint compatibility of loop-closure candidates (spg_graph_compatible_candidates, spg_ctx_max_clique; csrc/spg_compat.inc:
sp_compat_init_kernel / _pair_kernel / _verify_kernel, sp_clique_seed_kernel / _write_kernel) against the numpy rule of
tests/compat_ref.py.
CPU: block elimination and the block-Cholesky recurrence equal the dense d2, d2_ij >= max(d2_i, d2_j), greedy_clique returns
maximal cliques, the fixtures are decidable, the argument contract on an injected backend, the ABI and the bindings, the
quantile table, the C++ demo compiles.
GPU: max_clique against greedy_clique over word boundaries; the chain fixtures (SE2, SE3, both gauges) against the
reference; an independent path through jointMarginalCovariance; the aliased group that the individual gate lets through; the
earlier calls unchanged.

Bounds (derived, not measured). With Omega_i = L_i L_i^T, U_i = L_i^T A_i and w_i = L_i^T e_i, d2(S) = w_S^T M_SS^-1 w_S with
M_SS = I + U_S Sigma U_S^T >= I, so ||M_SS^-1||2 <= 1 and to first order |delta d2(S)| <= |w_S|^2 ||delta M_SS||2. A block
of M_SS is L_i^T C_ij L_j with C_ij = J_i Sigma_(ai bi),(aj bj) J_j^T, held to beta_ij = ||J_i||inf ||J_j||inf 1e-9
max|Sigma| + 1e-11 max|C_ij| (the convention of tests/test_relative_covariance.py: the project's bound on a covariance block
pushed through the Jacobians, plus the cap of the device geometry), so ||delta M_SS||2 <= |S| D max ||Omega||2 beta with beta
the largest beta_ij over the blocks of S, and

    bound(S) = |w_S|^2 |S| D max_i ||Omega_i||2 beta,        |w_S|^2 = sum over S of e_i^T Omega_i e_i

computed from the reference's own numbers (compat_ref.bound). d2_i: |S| = 1, pair_d2: |S| = 2, joint_d2 after p acceptances:
|S| = p. The fixtures are decidable when every decision the device has to reproduce lies at least 10 of its bounds from its
threshold: the gate of every candidate with a usable Omega, every eligible pair, every joint accept / reject, and the order of
the members by d2_i (neighbours in that order differ by 10 times the larger of their two bounds; identical records tie by
index). Smallest lead over 10 bounds (numpy alone): SE2 chain 6.6 (gauge 0) and 10.0 (gauge 17), SE3 chain 2.6 and 1.06.
Measured on an MI355X, worst error over its bound: d2 7.8e-10, pair_d2 2.9e-10, joint_d2 5.2e-11 (SE2); 1.9e-10, 5.8e-11,
1.2e-10 (SE3); the final joint distance through jointMarginalCovariance 1.6e-13 and 2.8e-14.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from sparsifyposegraph_amd import abi, chi2, lib
from sparsifyposegraph_amd.lib import SpgError
from tests import compat_ref as cr
from tests import oracle_lib, util
from tests import relative_ref as rr
from tests import select_ref as sr
from tests.test_candidate_selection import _at, _random_problem
from tests.test_covariance_blocks import _non_adjacent_pair, _small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")
_f64p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
EINVAL, ESTATE, ECAPACITY = -1, -7, -4
Q = 0.99


# ------------------------------------------------------------------------------------------------- the chain fixtures
# A loop of 60 poses (26 steps to the turn, so that poses 29 .. 34 pass where poses 3 .. 8 did) whose estimates are the
# integrated noisy odometry: every edge has zero residual and the drift between the two regions is several sigma of the
# candidates' own noise. CHAIN[d] = (seed, odometry sigma (m, rad), candidate sigma (m, rad), noise scale of the inliers),
# found by searching seeds and scales for decidability (test_chain_fixtures_are_decidable prints the leads).
CHAIN = {3: (1, (0.05, 0.01), (0.05, 0.02), 0.5), 6: (8, (0.035, 0.007), (0.05, 0.02), 0.5)}
REGION_A, REGION_B = range(3, 9), range(29, 35)
N_INLIER, N_ALIAS, N_INDEP = 18, 8, 6
ALIAS_OFFSET = {3: np.array([0.5, -0.35, 0.03]), 6: np.array([0.5, -0.35, 0.1, 0.01, -0.01, 0.015])}
INDEP_OFFSET = {3: np.array([0.5, 0.5, 0.04]), 6: np.array([0.5, 0.5, -0.2, 0.01, 0.01, 0.02])}
GROSS_OFFSET = {3: np.array([3.0, -3.0, 0.3]), 6: np.array([3.0, -3.0, 1.0, 0.05, 0.05, 0.15])}


def _delta(d, v):
    return np.asarray(v, np.float64) if d == 3 else rr.from_mqt(v)


def _sig(d, s):
    return np.array([s[0], s[0], s[1]]) if d == 3 else np.array([s[0]] * 3 + [s[1]] * 3)


@functools.lru_cache(maxsize=None)
def _chain(d):
    """(graph dict with the drifted estimates, true poses)"""
    seed, odo, _, _ = CHAIN[d]
    rng = np.random.default_rng(seed)
    n, period = 60, 26
    yaw = 2 * np.pi / period
    step = np.array([0.5, 0.0, yaw]) if d == 3 else rr.from_mqt([0.5, 0.0, 0.02, 0.0, 0.0, np.sin(0.5 * yaw)])
    x0 = np.zeros(3) if d == 3 else np.array([0, 0, 0, 0, 0, 0, 1.0])
    truth, est, z = [x0], [x0], []
    so = _sig(d, odo)
    for t in range(n - 1):
        truth.append(rr.compose(d, truth[t], step))
        z.append(rr.compose(d, step, _delta(d, rng.normal(size=d) * so)))
        est.append(rr.compose(d, est[t], z[t]))
    info = rr.upper(np.diag(1.0 / so ** 2))
    ij = [(t, t + 1) for t in range(n - 1)] + [(0, n - 1)]
    z.append(rr.between(d, est[0], est[n - 1]))
    g = {"pose_dim": d, "ids": np.arange(n, dtype=np.int32), "poses": np.array(est), "edge_ij": np.array(ij, np.int32),
         "edge_data": np.array([np.concatenate([m, info]) for m in z])}
    return g, np.array(truth)


def _chain_candidates(d, fid, lead=0):
    """The candidates of a chain fixture for the gauge fid: `lead` gross outliers first (only the individual gate removes
    them; they push the eligible candidates across index 64), then 18 inliers between the two regions (true relative pose
    plus a fraction of the candidates' sigma), 8 aliased closures with one common offset, 6 independent outliers (the
    offset with alternating sign), the fixed vertex as a and as b (inliers), the first inlier's record two more times, one
    candidate with an indefinite Omega and one gross outlier. Returns (ij, meas, info, groups): groups maps a name to the
    indices."""
    seed, _, cs, inl = CHAIN[d]
    _, truth = _chain(d)
    rng = np.random.default_rng(1000 * seed + fid)
    sc = _sig(d, cs)
    Om = np.diag(1.0 / sc ** 2)
    ij, meas, groups = [], [], {}

    def add(name, a, b, offset, noise):
        groups.setdefault(name, []).append(len(ij))
        ij.append((a, b))
        meas.append(rr.compose(d, rr.between(d, truth[a], truth[b]), _delta(d, offset + noise * rng.normal(size=d) * sc)))

    def pair():
        return int(rng.choice(list(REGION_A))), int(rng.choice(list(REGION_B)))
    keep, rng = rng, np.random.default_rng(77 + fid)         # a stream of their own: the other candidates do not depend on `lead`
    for _ in range(lead):
        add("lead", *pair(), GROSS_OFFSET[d] * (1 + rng.random()), 1.0)
    rng = keep
    for _ in range(N_INLIER):
        add("inlier", *pair(), np.zeros(d), inl)
    for _ in range(N_ALIAS):
        add("alias", *pair(), ALIAS_OFFSET[d], inl)
    for t in range(N_INDEP):
        add("indep", *pair(), INDEP_OFFSET[d] * (1 if t % 2 == 0 else -1), inl)
    other = 31 if fid != 31 else 30
    add("inlier", fid, other, np.zeros(d), inl)
    add("inlier", 5 if fid != 5 else 6, fid, np.zeros(d), inl)
    first = groups["inlier"][0]
    for _ in range(2):
        groups["inlier"].append(len(ij))
        groups.setdefault("copy", []).append(len(ij))
        ij.append(ij[first])
        meas.append(meas[first].copy())
    add("bad", *pair(), np.zeros(d), inl)
    add("gross", *pair(), GROSS_OFFSET[d], inl)
    info = np.tile(rr.upper(Om), (len(ij), 1))
    w, V = np.linalg.eigh(Om)
    w[0] = -0.5 * w[1]
    info[groups["bad"][0]] = rr.upper(V @ np.diag(w) @ V.T)
    groups["same"] = [first] + groups["copy"]
    return np.array(ij, np.int32), np.array(meas), info, groups


def _thresholds(d, k):
    return chi2.chi2_quantile(Q, d), chi2.chi2_quantile(Q, 2 * d), np.array(chi2.chi2_quantile_table(Q, d, k))


def _terms(d, poses, ids, fid, ij, meas, info):
    return sr.terms(d, {int(i): np.array(p) for i, p in zip(ids, poses)}, _at([int(i) for i in ids], fid), ij, meas, info)


@functools.lru_cache(maxsize=None)
def _chain_reference(d, fid, lead=0):
    """(ij, meas, info, groups, T, Sigma, reference run with k = n and the thresholds of significance 0.99), on the
    oracle's information of the fixture: computed once and shared by the tests."""
    g, _ = _chain(d)
    ij, meas, info, groups = _chain_candidates(d, fid, lead)
    Sig = np.linalg.inv(oracle_lib.OracleGraph.from_dict(g).information(fid))
    T = _terms(d, g["poses"], g["ids"], fid, ij, meas, info)
    gate, pair, joint = _thresholds(d, len(ij))
    return ij, meas, info, groups, T, Sig, cr.run(T, Sig, len(ij), gate, pair, joint)


def _leads(d, T, Sig, ref, groups):
    """Smallest |value - threshold| / (10 bound) per kind of decision, from the reference alone."""
    gate, pair, joint = _thresholds(d, len(T))
    out = {"gate": np.inf, "pair": np.inf, "joint": np.inf, "order": np.inf}
    b1 = {}
    for i, t in enumerate(T):
        if t["ok"]:
            b1[i] = cr.bound(T, Sig, [i])
            out["gate"] = min(out["gate"], abs(ref["d2"][i] - gate) / (10 * b1[i]))
    el = np.flatnonzero(ref["eligible"])
    for a, i in enumerate(el):
        for j in el[a + 1:]:
            out["pair"] = min(out["pair"], abs(ref["pair_d2"][i, j] - pair) / (10 * cr.bound(T, Sig, [i, j])))
    S = []
    for i, t, p, ok in ref["tested"]:
        out["joint"] = min(out["joint"], abs(t - joint[p]) / (10 * cr.bound(T, Sig, S + [i])))
        if ok:
            S.append(i)
    for i, j in zip(ref["order"][:-1], ref["order"][1:]):
        if i in groups["same"] and j in groups["same"]:
            continue
        out["order"] = min(out["order"], abs(ref["d2"][i] - ref["d2"][j]) / (10 * max(b1[i], b1[j])))
    return out


GAUGES = (0, 17)


# ------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("d", [3, 6])
def test_block_elimination_equals_the_dense_distance(d):
    """Random SPD H over 8 poses, 12 candidates (one with the fixed vertex): the pair distance by block elimination (i first)
    and every prefix distance of the block-Cholesky recurrence equal the literal d2(S) to 1e-10 (relative), and
    d2_ij >= max(d2_i, d2_j) minus rounding."""
    H, T = _random_problem(d, seed=20 + d)
    Sig = np.linalg.inv(H)
    one = [cr.dense_d2(T, Sig, [i]) for i in range(len(T))]
    for i in range(len(T)):
        for j in range(i + 1, len(T)):
            want = cr.dense_d2(T, Sig, [i, j])
            assert cr.pair_by_elimination(T, Sig, i, j) == pytest.approx(want, rel=1e-10)
            assert cr.pair_by_elimination(T, Sig, j, i) == pytest.approx(want, rel=1e-10)
            assert want >= max(one[i], one[j]) * (1 - 1e-12)
    order = [4, 0, 7, 2, 9, 11]
    seq = cr.sequential_by_cholesky(T, Sig, order)
    for p in range(len(order)):
        assert seq[p] == pytest.approx(cr.dense_d2(T, Sig, order[:p + 1]), rel=1e-10)
    assert np.all(np.diff(seq) >= 0)


def _random_graph(n, seed, p=0.5):
    rng = np.random.default_rng(seed)
    a = np.triu(rng.random((n, n)) < p, 1)
    return a | a.T


def test_greedy_clique_returns_maximal_cliques():
    for n, seed in ((1, 0), (2, 1), (17, 2), (40, 3), (90, 4)):
        adj = _random_graph(n, seed)
        R, s = cr.greedy_clique(adj)
        assert R[0] == s and len(set(R)) == len(R)
        assert all(adj[a, b] for a in R for b in R if a != b)
        assert not any(all(adj[v, u] for u in R) for v in range(n) if v not in R)      # no vertex extends it
    assert cr.greedy_clique(np.zeros((5, 5), bool)) == ([0], 0)
    assert cr.greedy_clique(np.zeros((0, 0), bool)) == ([], -1)
    assert cr.greedy_clique(np.ones((4, 4), bool) & ~np.eye(4, dtype=bool)) == ([0, 1, 2, 3], 0)
    assert cr.greedy_clique(_random_graph(9, 5), eligible=np.zeros(9, bool)) == ([], -1)


@pytest.mark.parametrize("d", [3, 6])
@pytest.mark.parametrize("lead", [0, 32])
def test_chain_fixtures_are_decidable(d, lead):
    """A condition on the inputs of the GPU tests, from the reference alone: in both gauges every gate, every eligible pair,
    every joint decision and the stage-3 order lie at least 10 bounds from their thresholds; the consistent set and the
    accepted sequence are exactly the inlier group; at least three outliers pass the individual gate (the regime in which the
    feature matters); and of the rest, only the gross outliers are gated and the indefinite Omega is reported."""
    for fid in GAUGES:
        ij, meas, info, groups, T, Sig, ref = _chain_reference(d, fid, lead)
        leads = _leads(d, T, Sig, ref, groups)
        print(f"SE{2 if d == 3 else 3} chain, gauge {fid}, {len(ij)} candidates: smallest lead / (10 bounds) " +
              ", ".join(f"{k} {v:.2e}" for k, v in leads.items()))
        assert min(leads.values()) >= 1.0, leads
        assert sorted(ref["clique"]) == sorted(groups["inlier"]) and sorted(ref["compatible"]) == sorted(groups["inlier"])
        outliers = groups["alias"] + groups["indep"]
        assert sum(bool(ref["eligible"][i]) for i in outliers) >= 3
        gated = np.flatnonzero(ref["status"] == cr.GATED)
        assert set(groups["gross"] + groups.get("lead", [])) <= set(gated) and not set(gated) & set(groups["inlier"])
        assert ref["status"][groups["bad"][0]] == cr.INFO_NOT_PD
        same = groups["same"]
        pos = [ref["order"].index(i) for i in same]
        assert pos == list(range(pos[0], pos[0] + 3))                                  # the copies tie and go by index


def test_abi_and_bindings_cover_the_compatibility():
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    L = C.CDLL(lib.LIB_PATH)
    for name in ("spg_graph_compatible_candidates", "spg_ctx_max_clique"):
        assert name in lib.SYMBOLS and hasattr(L, name)
    assert abi.CAND_INCOMPATIBLE == 4 == cr.INCOMPATIBLE and (cr.SCORED, cr.INFO_NOT_PD, cr.GATED, cr.SELECTED) == (0, 1, 2, 3)
    assert C.sizeof(abi.CompatStats) == C.sizeof(abi.CovSolveStats) + 48
    assert set(abi.CompatStats().asdict()) >= {"endpoints", "eligible", "consistent_pairs", "clique_size", "seed", "pair_seconds", "clique_seconds",
                                               "verify_seconds", "solve_seconds", "device_seconds"}
    assert callable(GraphWrapperHIP.compatibleCandidates) and callable(lib.Context.max_clique)
    hdr = open(os.path.join(ROOT, "include", "spg.h")).read()
    assert "SPG_CAND_INCOMPATIBLE = 4" in hdr and "spg_compat_stats" in hdr and "each unordered pair is computed once" in hdr.lower()
    assert "compatibleCandidates" in open(os.path.join(ROOT, "include", "spg_graph_wrapper.hpp")).read()
    stubs = open(os.path.join(ROOT, "tools", "asan_stubs.cpp")).read()
    assert "hip_sparse_compat" in stubs and "hip_max_clique" in stubs


def test_quantile_table_equals_the_single_quantile():
    for q, step in ((0.99, 3), (0.99, 6), (0.95, 6)):
        table = chi2.chi2_quantile_table(q, step, 300)
        assert len(table) == 300 and np.all(np.diff(table) > 0)
        for p in (1, 2, 3, 10, 77, 300):
            assert table[p - 1] == pytest.approx(chi2.chi2_quantile(q, step * p), rel=1e-10)
    assert chi2.chi2_quantile_table(0.99, 3, 0) == []
    assert chi2.chi2_quantile_table(0.99, 6, 1)[0] == pytest.approx(16.8119, abs=5e-5)
    with pytest.raises(ValueError):
        chi2.chi2_quantile_table(1.0, 3, 2)


def test_compat_checks_arguments_before_the_backend():
    """On an injected (CPU) context, as spg_graph_select_candidates: the size queries answer; k = 0 and n = 0 return 0; an
    unknown id, a == b, an unknown fixed vertex, a non-finite measurement, k < 0, pair_max_d2 <= 0, short clique / pair
    capacities and an active stepwise marginalisation are SPG_EINVAL with their word; more than 16 384 candidates are
    SPG_ECAPACITY; a call that would compute is SPG_ESTATE (no CPU fallback); the Python layer raises."""
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
    sel, jd, clq, d2, deg, status, pd = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int32), \
        np.zeros(n, np.int32), np.zeros((n, n))
    f = lambda x: x.ctypes.data_as(_f64p)  # noqa: E731
    i = lambda x: x.ctypes.data_as(_i32p)  # noqa: E731
    err = lambda: L.spg_last_error(ictx.h).decode()  # noqa: E731

    def compat(ij, r, cnt, k, cap, fid=-1, h=a.h, pair_max=16.8, clique_cap=n, pair_cap=n * n):
        return L.spg_graph_compatible_candidates(h, fid, i(ij), f(r), cnt, k, 0.0, pair_max, None, i(sel), f(jd), cap, i(clq), clique_cap, f(d2), i(deg),
                                                 i(status), f(pd), pair_cap, None)
    # size queries, k = 0, n = 0
    assert compat(pairs, rec, n, 2, 0) == 2 and compat(pairs, rec, n, 2, 1) == 2 and compat(pairs, rec, n, 9, 0) == n
    assert L.spg_graph_compatible_candidates(a.h, -1, i(pairs), f(rec), n, 3, 0.0, 16.8, None, None, None, 99, None, 0, None, None, None, None, 0, None) == 3
    assert compat(pairs, rec, n, 0, n) == 0 and compat(pairs, rec, 0, 3, n) == 0
    # no HIP backend
    st = abi.CompatStats()
    assert compat(pairs, rec, n, 2, 2) == ESTATE and "HIP backend" in err()
    assert L.spg_graph_compatible_candidates(a.h, -1, i(pairs), f(rec), n, n, 11.3, 16.8, f(jd), i(sel), f(jd), n, None, 0, None, None, None, None, 0,
                                             C.byref(st)) == ESTATE
    # invalid arguments, answered before the backend
    unknown = np.array([int(ids[0]), 999999], np.int32)
    same = np.array([e0[0], e0[0]], np.int32)
    for bad, word in ((unknown, "999999"), (same, "same")):
        assert compat(bad, rec, 1, 1, 1) == EINVAL and word in err() and "pair 0" in err() and "spg_graph_compatible_candidates" in err()
    assert compat(pairs, rec, n, 2, 2, fid=999999) == EINVAL and "fixed vertex" in err()
    assert compat(pairs, rec, n, -1, 2) == EINVAL and "negative" in err()
    for bad_pm in (0.0, -1.0, np.nan):
        assert compat(pairs, rec, n, 2, 2, pair_max=bad_pm) == EINVAL and "pair_max_d2" in err()
    assert compat(pairs, rec, n, 2, 2, clique_cap=n - 1) == EINVAL and "clique_cap" in err()
    assert compat(pairs, rec, n, 2, 2, pair_cap=n * n - 1) == EINVAL and "pair_cap" in err()
    for bad_value in (np.nan, np.inf):
        r2 = rec.copy()
        r2[2, 1] = bad_value
        assert compat(pairs, r2, n, 2, 2) == EINVAL
        assert "pair 2" in err() and f"({na[0]}, {na[1]})" in err() and "finite" in err()
    r2 = rec.copy()
    r2[1, D:] = np.nan          # a non-finite information is a status of the candidate, not an argument error
    assert compat(pairs, r2, n, 2, 0) == 2
    assert L.spg_graph_compatible_candidates(a.h, -1, i(pairs), None, n, 2, 0.0, 16.8, None, i(sel), f(jd), 2, None, 0, None, None, None, None, 0,
                                             None) == EINVAL
    # capacity: more candidates than the consistency graph holds, before the backend
    big = np.ascontiguousarray(np.tile(pairs[1], (16385, 1)))
    bigrec = np.ascontiguousarray(np.tile(rec[0], (16385, 1)))
    assert L.spg_graph_compatible_candidates(a.h, -1, i(big), f(bigrec), 16385, 2, 0.0, 16.8, None, i(sel), f(jd), 2, None, 0, None, None, None, None, 0,
                                             None) == ECAPACITY and "16384" in err()
    # an active stepwise marginalisation
    g, which, opts, *_ = util.load_golden("intel_nfr_tree_sp3")
    sub2, w = util.prefix_graph(g, which, 30)
    b = GraphWrapperHIP.from_dict(sub2, ctx=ictx)
    b.begin(w, opts, 0, 1)
    assert compat(pairs, rec, n, 2, 2, h=b.h) == EINVAL and "active" in err()
    # the Python layer
    with pytest.raises(SpgError, match="HIP backend"):
        a.compatibleCandidates(pairs, rec[:, :D], rec[:, D:], 2)
    with pytest.raises(SpgError, match="same"):
        a.compatibleCandidates([same], rec[:1, :D], rec[:1, D:], 1)
    with pytest.raises(SpgError, match="negative"):
        a.compatibleCandidates(pairs, rec[:, :D], rec[:, D:], -1)
    with pytest.raises(SpgError, match="pair_max_d2"):
        a.compatibleCandidates(pairs, rec[:, :D], rec[:, D:], 2, pair_max_d2=0.0)
    with pytest.raises(ValueError):
        a.compatibleCandidates(pairs, rec[:, :D], rec[:, D:-1], 2)
    with pytest.raises(ValueError):
        a.compatibleCandidates(pairs, rec[:, :D], rec[:, D:], 3, joint_max_d2=[1.0])
    got = a.compatibleCandidates(pairs, rec[:, :D], rec[:, D:], 0)
    assert len(got["compatible"]) == 0 and len(got["joint_d2"]) == 0 and got["d2"].shape == (n,) and len(got["clique"]) == 0
    assert got["max_d2"] == pytest.approx(11.3449, abs=5e-5) and got["pair_max_d2"] == pytest.approx(16.8119, abs=5e-5)
    got = a.compatibleCandidates(np.zeros((0, 2), np.int32), np.zeros((0, D)), np.zeros((0, D * (D + 1) // 2)))      # n = 0
    assert len(got["compatible"]) == 0 and got["status"].shape == (0,) and got["degree"].shape == (0,)


def _words(adj):
    n = len(adj)
    nw = max((n + 63) // 64, 1)
    bits = np.zeros((n, nw * 64), np.uint8)
    bits[:, :n] = adj
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8").reshape(n, nw)


def test_max_clique_rejects_what_is_not_a_consistency_graph():
    """spg_ctx_max_clique on an injected context: an asymmetric matrix, a set diagonal bit and bits at or beyond n are
    SPG_EINVAL with their word; n = 0 returns 0; more than 16 384 vertices are SPG_ECAPACITY; a graph that passes is
    SPG_ESTATE (no CPU fallback); Context.max_clique raises."""
    ictx = oracle_lib.injected_context()
    L = ictx.L
    err = lambda: L.spg_last_error(ictx.h).decode()  # noqa: E731
    u64 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731
    out, seed = np.zeros(70, np.int32), C.c_int32(0)

    def call(words, n):
        return L.spg_ctx_max_clique(ictx.h, n, u64(words), out.ctypes.data_as(_i32p), 70, C.byref(seed))
    good = _random_graph(70, 11)
    assert call(_words(good), 70) == ESTATE and "HIP backend" in err()
    asym = good.copy()
    asym[3, 66] = not asym[66, 3]
    assert call(_words(asym), 70) == EINVAL and "symmetric" in err()
    diag = good.copy()
    diag[65, 65] = True
    assert call(_words(diag), 70) == EINVAL and "diagonal" in err() and "65" in err()
    stray = _words(good).copy()
    stray[5, 1] |= np.uint64(1) << np.uint64(6)          # bit 70 of row 5
    assert call(stray, 70) == EINVAL and "beyond n" in err()
    assert call(_words(good), 0) == 0 and L.spg_ctx_max_clique(ictx.h, -1, None, None, 0, None) == EINVAL
    assert L.spg_ctx_max_clique(ictx.h, 3, None, None, 0, None) == EINVAL
    assert call(np.zeros((1, 1), np.uint64), 16385) == ECAPACITY
    with pytest.raises(SpgError, match="symmetric"):
        ictx.max_clique(asym)
    with pytest.raises(ValueError):
        ictx.max_clique(np.zeros((3, 4), bool))
    none = ictx.max_clique(np.zeros((0, 0), bool))
    assert len(none["clique"]) == 0 and none["seed"] == -1


def _build_demo(tmp_path):
    exe = str(tmp_path / "compat_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "compat_demo.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_compat_demo_compiles(tmp_path):
    out = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr


# ------------------------------------------------------------------------------------------------------- GPU
def _clique_graphs(n):
    """name -> boolean matrix: the graphs of the max_clique test at size n"""
    rng = np.random.default_rng(100 + n)
    out = {"empty": np.zeros((n, n), bool), "complete": np.ones((n, n), bool) & ~np.eye(n, dtype=bool)}
    planted = _random_graph(n, 200 + n)
    c = min(n, 12)
    lo = max(0, min(64 - c // 2, n - c))                   # straddles the first word boundary where n allows
    planted[lo:lo + c, lo:lo + c] = True
    np.fill_diagonal(planted, False)
    out["planted"] = planted
    two = np.zeros((n, n), bool)
    h = n // 2
    perm = rng.permutation(n)
    for part in (perm[:h], perm[h:2 * h]):
        two[np.ix_(part, part)] = True
    np.fill_diagonal(two, False)
    out["two equal cliques"] = two
    late = np.zeros((n, n), bool)                          # a path over the low indices, the clique at the high ones
    c = max(n // 3, 1)
    for v in range(n - c - 1):
        late[v, v + 1] = late[v + 1, v] = True
    late[n - c:, n - c:] = True
    if n - c - 1 >= 0:
        late[n - c - 1, n - c] = late[n - c, n - c - 1] = True
    np.fill_diagonal(late, False)
    out["a later seed"] = late
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 257])
def test_max_clique_equals_greedy_clique(n, hip_ctx):
    """Context.max_clique against compat_ref.greedy_clique: size, seed and ordered members are equal on the empty and the
    complete graph, G(n, 1/2) with a planted clique across a word boundary, two disjoint cliques of equal size (the tie goes
    to the lowest seed) and a graph where only a later seed reaches the largest clique."""
    for name, adj in _clique_graphs(n).items():
        want, seed = cr.greedy_clique(adj)
        got = hip_ctx.max_clique(adj)
        assert got["clique"].tolist() == want and got["seed"] == seed, (n, name, got, want, seed)
        if name == "a later seed" and n >= 6:
            assert seed > 0 and len(want) == max(n // 3, 1)
        if name == "two equal cliques" and n >= 2:
            assert len(want) == n // 2


def _device_graph(d, hip_ctx):
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, _ = _chain(d)
    return GraphWrapperHIP.from_dict(g, ctx=hip_ctx)


def _check_values(T, Sig, ref, got, what):
    """d2, pair_d2 and joint_d2 of a device run against the reference within their bounds; returns worst error / bound"""
    worst = {"d2": 0.0, "pair_d2": 0.0, "joint_d2": 0.0}
    n = len(T)
    assert np.array_equal(np.isnan(got["d2"]), np.isnan(ref["d2"]))
    for i in range(n):
        if np.isfinite(ref["d2"][i]):
            r = abs(got["d2"][i] - ref["d2"][i]) / cr.bound(T, Sig, [i])
            worst["d2"] = max(worst["d2"], r)
            assert r <= 1.0, (what, "d2", i, r)
    if "pair_d2" in got:
        pd = got["pair_d2"]
        assert np.array_equal(pd, pd.T, equal_nan=True)                       # exactly symmetric
        assert np.array_equal(np.isnan(pd), np.isnan(ref["pair_d2"]))
        el = np.flatnonzero(ref["eligible"])
        assert np.array_equal(pd[el, el], got["d2"][el])
        for a, i in enumerate(el):
            for j in el[a + 1:]:
                r = abs(pd[i, j] - ref["pair_d2"][i, j]) / cr.bound(T, Sig, [i, j])
                worst["pair_d2"] = max(worst["pair_d2"], r)
                assert r <= 1.0, (what, "pair_d2", i, j, r)
    assert len(got["joint_d2"]) == len(ref["joint_d2"])
    for p in range(len(ref["joint_d2"])):
        r = abs(got["joint_d2"][p] - ref["joint_d2"][p]) / cr.bound(T, Sig, list(ref["compatible"][:p + 1]))
        worst["joint_d2"] = max(worst["joint_d2"], r)
        assert r <= 1.0, (what, "joint_d2", p, r)
    print(f"{what}: worst error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
@pytest.mark.parametrize("lead", [0, 32])
def test_chain_fixtures_equal_the_reference(d, lead, hip_ctx):
    """The chain fixture (38 candidates; lead = 32: 70 candidates, the eligible ones across index 64) in both gauges at significance 0.99:
    status, degree, the consistent set and the accepted sequence equal the reference exactly; d2, pair_d2 and joint_d2 are
    within their bounds; pair_d2 is exactly symmetric with d2 on its diagonal; the stats agree with the outputs. Measured
    worst error / bound: d2 7.8e-10, pair_d2 2.9e-10, joint_d2 1.2e-10 (module docstring)."""
    hg = _device_graph(d, hip_ctx)
    for fid in GAUGES:
        ij, meas, info, groups, T, Sig, ref = _chain_reference(d, fid, lead)
        got = hg.compatibleCandidates(ij, meas, info, significance=Q, pairs=True, fixed_id=fid)
        what = f"SE{2 if d == 3 else 3} chain, gauge {fid}, n = {len(ij)}"
        assert np.array_equal(got["status"], ref["status"]), (what, got["status"], ref["status"])
        assert np.array_equal(got["degree"], ref["degree"]), what
        assert got["clique"].tolist() == ref["clique"], what
        assert np.array_equal(got["compatible"], ref["compatible"]), what
        assert sorted(got["compatible"].tolist()) == sorted(groups["inlier"])
        _check_values(T, Sig, ref, got, what)
        s = hg.last_covariance_stats
        assert s["clique_size"] == len(ref["clique"]) and s["seed"] == ref["seed"] and s["eligible"] == int(ref["eligible"].sum())
        assert s["consistent_pairs"] == int(ref["adj"].sum()) // 2 and s["endpoints"] == len({int(v) for v in ij.ravel()} - {fid})
        assert s["pair_seconds"] > 0 and s["clique_seconds"] > 0 and s["verify_seconds"] > 0
        assert s["pair_seconds"] + s["clique_seconds"] + s["verify_seconds"] < s["device_seconds"]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_small_lists_no_joint_gate_and_early_stop(d, hip_ctx):
    """On the chain fixture, gauge 0: n = 1 and n = 2 (the first two inliers); without joint thresholds the consistent set is
    accepted in (d2, index) order up to k, the identical records in index order; a k below the size of the set stops early
    and leaves the members never examined SPG_CAND_SCORED; a joint gate only the first member passes marks the others
    SPG_CAND_INCOMPATIBLE; an individual gate nobody passes gives an empty set, seed -1 and nothing accepted."""
    hg = _device_graph(d, hip_ctx)
    fid = 0
    ij, meas, info, groups, T, Sig, ref = _chain_reference(d, fid)
    gate, pair, joint = _thresholds(d, len(ij))
    one = hg.compatibleCandidates(ij[:1], meas[:1], info[:1], significance=Q, pairs=True, fixed_id=fid)
    assert one["compatible"].tolist() == [0] and one["clique"].tolist() == [0] and one["status"].tolist() == [abi.CAND_SELECTED]
    assert one["degree"].tolist() == [0] and one["pair_d2"].shape == (1, 1) and one["pair_d2"][0, 0] == one["d2"][0] == one["joint_d2"][0]
    assert abs(one["d2"][0] - ref["d2"][0]) <= cr.bound(T, Sig, [0])
    two = hg.compatibleCandidates(ij[:2], meas[:2], info[:2], significance=Q, pairs=True, fixed_id=fid)
    first = [0, 1] if (ref["d2"][0], 0) < (ref["d2"][1], 1) else [1, 0]
    assert two["compatible"].tolist() == first and two["clique"].tolist() == [0, 1] and two["degree"].tolist() == [1, 1]
    assert abs(two["joint_d2"][1] - ref["pair_d2"][0, 1]) <= cr.bound(T, Sig, [0, 1]) and two["pair_d2"][0, 1] == two["pair_d2"][1, 0]
    assert abs(two["joint_d2"][1] - two["pair_d2"][0, 1]) <= cr.bound(T, Sig, [0, 1])
    # no joint gate: the set in stage-3 order, up to k
    free = hg.compatibleCandidates(ij, meas, info, significance=Q, joint_max_d2=False, fixed_id=fid)
    assert free["compatible"].tolist() == ref["order"] and free["joint_max_d2"] is None
    k = 5
    few = hg.compatibleCandidates(ij, meas, info, k=k, significance=Q, joint_max_d2=False, fixed_id=fid)
    assert few["compatible"].tolist() == ref["order"][:k] and len(few["joint_d2"]) == k
    rest = [i for i in ref["clique"] if i not in ref["order"][:k]]
    assert np.all(few["status"][rest] == abi.CAND_SCORED) and np.all(few["status"][ref["order"][:k]] == abi.CAND_SELECTED)
    assert few["clique"].tolist() == ref["clique"] and np.array_equal(few["joint_d2"], free["joint_d2"][:k])
    # with the joint gate and the same k: the reference's first k acceptances
    gated = hg.compatibleCandidates(ij, meas, info, k=k, significance=Q, fixed_id=fid)
    assert gated["compatible"].tolist() == ref["compatible"][:k].tolist() and np.array_equal(gated["joint_max_d2"], joint[:k])
    # a joint gate nobody passes twice: the first member is accepted (threshold above its d2), every other one is rejected
    tight = np.concatenate([[gate], np.full(len(ij) - 1, 1e-3)])
    rej = hg.compatibleCandidates(ij, meas, info, significance=Q, joint_max_d2=tight, fixed_id=fid)
    assert rej["compatible"].tolist() == ref["order"][:1] and np.all(rej["status"][ref["order"][1:]] == abi.CAND_INCOMPATIBLE)
    # a gate nobody passes (every d2 of the fixture is above 1e-3): no seed, an empty set, nothing accepted
    assert np.nanmin(ref["d2"]) > 1e-3
    none = hg.compatibleCandidates(ij, meas, info, significance=Q, max_d2=1e-6, fixed_id=fid)
    s = hg.last_covariance_stats
    assert len(none["compatible"]) == 0 and len(none["clique"]) == 0 and s["seed"] == -1 and s["clique_size"] == 0 and s["eligible"] == 0
    assert np.all(none["degree"] == 0) and set(none["status"].tolist()) == {abi.CAND_GATED, abi.CAND_INFO_NOT_PD}


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_final_joint_distance_through_the_joint_marginal_covariance(d, hip_ctx):
    """Independent of the compatibility kernels: the final joint_d2 equals w_S^T M_SS^-1 w_S assembled in numpy from the
    device's own jointMarginalCovariance of the accepted candidates' endpoints, within the joint bound."""
    hg = _device_graph(d, hip_ctx)
    for fid in GAUGES:
        ij, meas, info, groups, T, Sig, ref = _chain_reference(d, fid)
        got = hg.compatibleCandidates(ij, meas, info, significance=Q, fixed_id=fid)
        S = got["compatible"].tolist()
        ends = sorted({int(v) for i in S for v in ij[i]} - {fid})
        at = {v: k for k, v in enumerate(ends)}
        Sd = hg.jointMarginalCovariance(ends, fixed_id=fid)
        U, w = [], []
        for i in S:
            A = np.zeros((d, d * len(ends)))
            for slot, v in enumerate(int(x) for x in ij[i]):
                if v != fid:
                    A[:, at[v] * d:(at[v] + 1) * d] = T[i]["J"][:, slot * d:(slot + 1) * d]
            Lc = np.linalg.cholesky(T[i]["Om"])
            U.append(Lc.T @ A)
            w.append(Lc.T @ T[i]["e"])
        U, w = np.vstack(U), np.concatenate(w)
        want = float(w @ np.linalg.solve(np.eye(len(w)) + U @ Sd @ U.T, w))
        b = cr.bound(T, Sig, S)
        print(f"SE{2 if d == 3 else 3} chain, gauge {fid}: joint d2 {got['joint_d2'][-1]:.12g}, through jointMarginalCovariance {want:.12g}, "
              f"difference / bound {abs(got['joint_d2'][-1] - want) / b:.2e}")
        assert abs(got["joint_d2"][-1] - want) <= b


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 6])
def test_aliased_group_passes_the_gate_but_not_the_joint_test(d, hip_ctx):
    """The point of the feature, and the regression: with the same max_d2, selectCandidates selects at least one outlier of
    the chain fixture, and compatibleCandidates returns exactly the inlier group; scoreCandidates' and selectCandidates'
    results are bit for bit the same before and after the compatibleCandidates call, and the graph is untouched."""
    hg = _device_graph(d, hip_ctx)
    fid = 0
    ij, meas, info, groups, T, Sig, ref = _chain_reference(d, fid)
    gate, _, _ = _thresholds(d, len(ij))
    k = len(groups["inlier"])
    score0 = hg.scoreCandidates(ij, meas, info, fixed_id=fid)
    sel0 = hg.selectCandidates(ij, meas, info, k, max_d2=gate, fixed_id=fid)
    e0, v0 = hg.edges(), hg.vertices()
    got = hg.compatibleCandidates(ij, meas, info, significance=Q, fixed_id=fid)
    score1 = hg.scoreCandidates(ij, meas, info, fixed_id=fid)
    sel1 = hg.selectCandidates(ij, meas, info, k, max_d2=gate, fixed_id=fid)
    e1, v1 = hg.edges(), hg.vertices()
    outliers = set(groups["alias"] + groups["indep"])
    assert len(set(sel0["selected"].tolist()) & outliers) >= 1
    assert sorted(got["compatible"].tolist()) == sorted(groups["inlier"]) and not set(got["compatible"].tolist()) & outliers
    for key in score0:
        assert np.array_equal(score0[key], score1[key], equal_nan=True), key
    for key in sel0:
        assert np.array_equal(sel0[key], sel1[key], equal_nan=True), key
    for key in e0:
        assert np.array_equal(e0[key], e1[key]), key
    assert np.array_equal(v0[0], v1[0]) and np.array_equal(v0[1], v1[1])
    # the individual distances are those of scoreCandidates within the single bound (another set of solved columns)
    for i in np.flatnonzero(np.isfinite(ref["d2"])):
        assert abs(got["d2"][i] - score0["d2"][i]) <= 2 * cr.bound(T, Sig, [int(i)])


@pytest.mark.gpu
def test_cpp_facade_compatibility_matches_python(tmp_path, hip_ctx):
    """tests/cpp/compat_demo.cpp runs the call through the façade on a small sphere; the accepted indices and joint distances
    equal the Python binding's bit for bit."""
    from sparsifyposegraph_amd import g2o_io
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = g2o_io.synth_sphere(n_poses=200, ring=20)
    path = str(tmp_path / "s200.g2o")
    g2o_io.write_g2o(path, g)
    out = subprocess.run([_build_demo(tmp_path), path, "12", "40.0", str(tmp_path / "cpp.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and "compatibility ok" in out.stdout, out.stdout + out.stderr
    cpp = np.loadtxt(str(tmp_path / "cpp.txt")).reshape(-1, 2)
    hg = GraphWrapperHIP.load(path, ctx=hip_ctx)
    ids = [int(i) for i in hg.vertices()[0]]
    n = len(ids)
    pairs = np.array([(ids[i], ids[n - 1 - i]) for i in range(n // 2)], np.int32)
    rel, _ = hg.relativeCovariances(pairs)
    e = hg.edges()
    k = next(k for k in range(len(e["kind"])) if ids[0] in e["vert_ids"][e["vert_off"][k]:e["vert_off"][k + 1]])
    info = e["data"][e["data_off"][k] + 7:e["data_off"][k + 1]]
    h = len(pairs) // 2
    meas = np.array([rel[i] if i < h else rel[(i + 1) % len(pairs)] for i in range(len(pairs))])
    got = hg.compatibleCandidates(pairs, meas, np.tile(info, (len(pairs), 1)), k=12, max_d2=0.0, pair_max_d2=40.0, joint_max_d2=False)
    assert len(cpp) == len(got["compatible"]) > 0
    assert np.array_equal(cpp[:, 0].astype(np.int32), got["compatible"]) and np.array_equal(cpp[:, 1], got["joint_d2"])
