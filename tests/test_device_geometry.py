"""The device pose geometry (csrc/spg_dev_geom.hpp: R_to_quat, dq_dR, se3_edge_jac, iso_from_mqt, normalize_theta,
se2_between, se2_edge_jac) at large rotations, against the multiprecision reference tests/geom_ref.py — through the public
ABI only, on graphs of 2-8 vertices. The fixture tests/golden/geometry_cases.npz (tests/golden/make_geometry_cases.py)
holds the named case table and the float64-rounded reference outputs; the GPU tests read nothing else.

Case table: every case is (Xi, Xj, Z, Omega) with a random SPD Omega of condition 1e3. SE3: the error rotation
E = Z^-1 Xi^-1 Xj in each of the four extraction branches, on the borders tr(E) = +-1e-3, +-1e-9 and two equal diagonal
entries, with w < 0 before normalisation, exact half-turns, zero error at a large relative rotation (the new-edge case)
and translations of order 1e3. SE2: heading differences at +-(pi - 1e-12) and exactly +-pi, stored headings outside
[-pi, pi), errors that wrap at the first or only at the second normalize_theta.

Half-turns (qw == 0): the kernel, like the oracle (oracle/ref_geom.hpp: R_to_quat flips on q[3] < 0, dq_dR on qw <= 0),
keeps +q in the error and negates the Jacobian. Cases with |qw| < 1e-3 are therefore left out of the
sign-sensitive checks (err and J on the CPU); they are exactly SIGN_EXCLUDED below, 4 of 49. chi2 = e^T Omega e and
H = J^T Omega J do not depend on that sign when Omega has no translation-rotation block — with such a block both do,
through the cross terms — so these four cases carry an Omega of two 3 x 3 blocks and are checked on chi2 and H everywhere.

Scale of a comparison: max |reference| of the quantity and case, but not less than 1 for err (the compact quaternion is
part of a UNIT quaternion, so an error of one fp64 ulp of 1 is the format's precision however small the vector part)
and not less than max |Omega| for chi2 (the chi2 of such a unit error): zero-error cases have err ~ 1e-17.

Tolerances (measured, not chosen): worst error of the fp64 oracle against the fixture over the whole table on that scale,
    err 2.01e-13 (lever_150_near_x)   J 7.00e-16 (lever_150_near_x)   H 1.36e-15 (border_diag_170_zx)
    chi2 1.83e-13 (lever_150_near_z)  between 4.44e-16 (sign_200_near_x)
recorded, rounded up, in ORACLE below and asserted on the CPU. err and chi2 are set by the lever-arm cases (|t| ~ 1e3: a
translation error of order 1 is a difference of numbers of order 1e3, eps * 1e3 = 2.2e-13 absolute); J, H and between sit
at a few ulp. The device runs the same formulas in another operation order and with FMA contraction and gets 8 x the
oracle's figure, never more than 1e-11 (DEVICE below):
    err 1.7e-12   J 5.7e-15   H 1.1e-14   chi2 1.5e-12   between 3.6e-15
The Mahalanobis term of the KLD passes through the Cholesky factor of a 30 x 30 information matrix: it takes util.RTOL,
the project's relative fp64 bound for KLD terms.
"""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from sparsifyposegraph_amd import abi
from tests import oracle_lib, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = dict(np.load(os.path.join(util.GOLDEN_DIR, "geometry_cases.npz")))

ORACLE = {"err": 2.1e-13, "J": 7.1e-16, "H": 1.4e-15, "chi2": 1.9e-13, "between": 4.5e-16}
DEVICE = {k: min(8 * v, 1e-11) for k, v in ORACLE.items()}
LM_STEPS = 12
SIGN_EXCLUDED = {"halfturn_x", "halfturn_y", "halfturn_z", "halfturn_111"}


def _P(a):
    import ctypes as C
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _cases(d):
    """[(name, dict of the case's inputs and reference outputs)]"""
    p = "se3_" if d == 6 else "se2_"
    keys = [k[len(p):] for k in FX if k.startswith(p) and k != p + "names"]
    return [(str(n), {k: FX[p + k][c] for k in keys}) for c, n in enumerate(FX[p + "names"])]


def _scale(kind, ref, omega=None):
    s = float(np.abs(ref).max())
    if kind in ("err", "between"):
        s = max(s, 1.0)
    if kind == "chi2":
        s = max(s, float(np.abs(omega).max()))
    return s


def _miss(kind, got, ref, omega=None):
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max()) / _scale(kind, np.asarray(ref), omega)


def _pair_graph(d, c):
    return {"pose_dim": d, "ids": np.array([1, 2], np.int32), "poses": np.array([c["xi"], c["xj"]]),
            "edge_ij": np.array([[1, 2]], np.int32), "edge_data": np.array([np.concatenate([c["z"], c["omega"]])])}


def _chain_graph(d, c):
    return {"pose_dim": d, "ids": np.array([0, 1, 2], np.int32), "poses": np.array([c["xa"], c["xi"], c["xj"]]),
            "edge_ij": np.array([[0, 1], [1, 2]], np.int32),
            "edge_data": np.array([np.concatenate([c["z_ai"], c["omega_ai"]]), np.concatenate([c["z"], c["omega"]])])}


def _drop(H, d, v):
    keep = [i for i in range(H.shape[0]) if i // d != v]
    return H[np.ix_(keep, keep)]


def _branch(q):
    """Extraction branch of the rotation of a unit quaternion (x, y, z, w): 'w' (tr > 0) or the largest diagonal entry;
    and the argument of the square root that branch takes."""
    x, y, z, w = q / np.linalg.norm(q)
    diag = np.array([1 - 2 * (y * y + z * z), 1 - 2 * (x * x + z * z), 1 - 2 * (x * x + y * y)])
    tr = diag.sum()
    if tr > 0:
        return "w", tr + 1.0
    i = int(np.argmax(diag))
    return "xyz"[i], 1.0 + 2 * diag[i] - tr


def _from_compact(v):
    return np.concatenate([v, [np.sqrt(1 - v @ v)]])


def _error_quat(c):
    from sparsifyposegraph_amd import g2o_io
    return g2o_io.quat_mul(g2o_io.quat_conj(c["z"][3:]), g2o_io.quat_mul(g2o_io.quat_conj(c["xi"][3:]), c["xj"][3:]))


# ---------------------------------------------------------------------------------------------------------- CPU
def test_fixture_is_what_the_reference_generates():
    """With mpmath present the fixture is regenerated and must equal the committed file bit for bit: inputs and reference
    outputs. (Without mpmath there is nothing to regenerate with: the committed file is then the only copy of the
    reference, and the oracle test below still checks it.)"""
    try:
        import mpmath  # noqa: F401
    except ImportError:
        return
    spec = importlib.util.spec_from_file_location("make_geometry_cases", os.path.join(util.GOLDEN_DIR, "make_geometry_cases.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    new = mk.generate()
    assert sorted(new) == sorted(FX)
    for k in sorted(new):
        assert np.array_equal(np.asarray(new[k]), FX[k]), k


def test_case_table_covers_what_it_claims():
    """The inputs are where the table says: every extraction branch and both outcomes of each sign test are met by the
    ERROR rotation, every square root of the extraction has an argument >= 1 (so no 1 / sqrt amplifies the rounding of E),
    the excluded half-turn cases are exactly those with |qw| < 1e-3 and at most 10 % of the table."""
    cases = _cases(6)
    seen = {}
    for name, c in cases:
        b, arg = _branch(_error_quat(c))
        assert arg >= 1.0 - 1e-12, (name, arg)
        seen.setdefault(b, []).append(name)
    assert set(seen) == {"w", "x", "y", "z"} and all(len(v) >= 5 for v in seen.values()), {k: len(v) for k, v in seen.items()}
    small = {name for name, c in cases if abs(c["ref_qw"]) < 1e-3}
    assert small == SIGN_EXCLUDED and len(small) <= 0.1 * len(cases)
    assert all(c["ref_qw"] == 0.0 for name, c in cases if name in small)
    # w < 0 before normalisation: the composed quaternion of the stored values has a negative w in a fair share of the table
    assert sum(_error_quat(c)[3] < 0 for _, c in cases) >= 10
    # borders: |tr(E)| as small as named
    for name, c in cases:
        if name.startswith("border_tr_"):
            q = _error_quat(c)
            tr = 4 * q[3] ** 2 / (q @ q) - 1
            want = float(name.split("_")[2].replace("p", "+").replace("m", "-"))
            assert tr == pytest.approx(want, rel=1e-3), (name, tr)
        if name.startswith("border_diag_"):
            x, y, z, w = _error_quat(c)
            diag = sorted([1 - 2 * (y * y + z * z), 1 - 2 * (x * x + z * z), 1 - 2 * (x * x + y * y)])
            assert diag[2] - diag[1] < 1e-12, (name, diag)
    # the graphs: absolute orientations of the ring and relative rotations of the star in all four branches
    assert {_branch(p[3:])[0] for p in FX["ring3_truth"]} == {"w", "x", "y", "z"}
    rel = {_branch(FX["star_ref_between"][a, b][3:])[0] for a in range(1, 5) for b in range(1, 5) if a != b}
    assert rel == {"w", "x", "y", "z"}
    assert {_branch(_from_compact(v[3:]))[0] for v in FX["kld_ref_diff"]} == {"w", "x", "y", "z"}
    th = FX["ring2_truth"][:, 2]
    assert (th > 3.0).sum() >= 2 and (th < -2.8).sum() >= 2


def test_oracle_matches_the_reference_over_the_table(oracle):
    """spgref_se3_edge / spgref_se2_edge / spgref_se*_between, and chi2() / information() of the oracle's graph, against the
    fixture over the whole table. The worst figures ARE the tolerances of this module (header): they may not exceed what is
    recorded there, and the device gets 8 x of it."""
    worst = {k: (0.0, "") for k in ORACLE}

    def note(kind, name, m):
        if m > worst[kind][0]:
            worst[kind] = (m, name)

    for d in (6, 3):
        for name, c in _cases(d):
            err, Ji, Jj, z = np.zeros(d), np.zeros((d, d)), np.zeros((d, d)), np.zeros(abi.pose_stride(d))
            if d == 6:
                oracle.spgref_se3_edge(_P(c["xi"]), _P(c["xj"]), _P(c["z"]), _P(err), _P(Ji), _P(Jj))
                oracle.spgref_se3_between(_P(c["xi"]), _P(c["xj"]), _P(z))
            else:
                oracle.spgref_se2_edge(_P(c["xi"]), _P(c["xj"]), _P(c["z"]), _P(err), _P(Ji), _P(Jj))
                oracle.spgref_se2_between(_P(c["xi"]), _P(c["xj"]), _P(z))
            if name not in SIGN_EXCLUDED:
                note("err", name, _miss("err", err, c["ref_err"]))
                note("J", name, max(_miss("J", Ji, c["ref_Ji"]), _miss("J", Jj, c["ref_Jj"])))
                note("between", name, _miss("between", z, c["ref_between"]))
                if d == 6:
                    assert z[6] >= 0 and abs(np.linalg.norm(z[3:]) - 1) < 1e-15
            og = oracle_lib.OracleGraph.from_dict(_pair_graph(d, c))
            note("chi2", name, _miss("chi2", og.chi2(1), c["ref_chi2"], c["omega"]))
            og = oracle_lib.OracleGraph.from_dict(_chain_graph(d, c))
            for v in range(3):
                note("H", name, _miss("H", og.information(v), _drop(c["ref_H"], d, v)))
    print("oracle against the multiprecision reference, worst over the table: " + ", ".join(f"{k} {m:.2e} ({n})" for k, (m, n) in worst.items()))
    for k, (m, n) in worst.items():
        assert m <= ORACLE[k], (k, m, n)


def _ring(d, poses):
    p = "ring3_" if d == 6 else "ring2_"
    return {"pose_dim": d, "ids": np.arange(8, dtype=np.int32), "poses": np.array(poses), "edge_ij": FX[p + "ij"], "edge_data": FX[p + "data"]}


def _same_poses(d, got, want, tol):
    got, want = np.array(got), np.array(want)
    if d == 6:
        sign = np.sign(np.sum(got[:, 3:] * want[:, 3:], axis=1))[:, None]
        return np.abs(got[:, :3] - want[:, :3]).max() < tol and np.abs(got[:, 3:] * sign - want[:, 3:]).max() < tol
    dth = np.angle(np.exp(1j * (got[:, 2] - want[:, 2])))
    return np.abs(got[:, :2] - want[:, :2]).max() < tol and np.abs(dth).max() < tol


@pytest.mark.parametrize("d", [6, 3])
def test_oracle_lm_recovers_the_ring_from_a_far_start(d):
    """The oracle on the graphs of the device tests below: noise-free ring, start 0.3 rad and 0.2 m from the truth."""
    p = "ring3_" if d == 6 else "ring2_"
    og = oracle_lib.OracleGraph.from_dict(_ring(d, FX[p + "start"]))
    st = og.optimize(50, 0)
    assert st["chi2_initial"] > 1.0 and st["chi2_final"] < 1e-16, st
    assert _same_poses(d, og.vertices()[1], FX[p + "truth"], 1e-9)


@pytest.mark.parametrize("turn", [0, 1, 2])
def test_oracle_lm_improves_the_ring_with_a_vertex_turned_by_150_degrees(turn):
    """The precondition of the device test below holds for the oracle alone: chi2 decreases from the turned start."""
    og = oracle_lib.OracleGraph.from_dict(_ring(6, FX["ring3_turned"][turn]))
    st = og.optimize(50, 0)
    assert st["chi2_final"] < st["chi2_initial"], st


# ---------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(params=["dense", "sparse"])
def solver_ctx(request, hip_ctx):
    solver = abi.SOLVER_DENSE if request.param == "dense" else abi.SOLVER_SPARSE
    hip_ctx.set_linear_solver(solver)
    yield hip_ctx, solver
    hip_ctx.set_linear_solver(abi.SOLVER_AUTO)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [6, 3])
def test_device_chi2_of_every_case(d, hip_ctx):
    """edge_chi2_kernel: R_to_quat (normalize_theta twice for SE2) on the error of every case, one 2-vertex graph each."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    bad, worst = [], (0.0, "")
    for name, c in _cases(d):
        got = GraphWrapperHIP.from_dict(_pair_graph(d, c), ctx=hip_ctx).chi2()
        m = _miss("chi2", got, c["ref_chi2"], c["omega"])
        print(f"chi2 {name}: device {got:.17g} reference {c['ref_chi2']:.17g} miss {m:.2e}")
        worst = max(worst, (m, name))
        if not m <= DEVICE["chi2"]:
            bad.append((name, m))
    print(f"worst {worst[0]:.2e} ({worst[1]}), bound {DEVICE['chi2']:.2e}")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("d", [6, 3])
def test_device_information_of_every_case(d, hip_ctx):
    """dense_assemble_kernel: Ji^T Omega Ji, Ji^T Omega Jj and Jj^T Omega Jj of every case in one call on the chain
    a - i - j (a - i a plain edge), with a, then i, then j held fixed."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    bad, worst = [], (0.0, "")
    for name, c in _cases(d):
        hg = GraphWrapperHIP.from_dict(_chain_graph(d, c), ctx=hip_ctx)
        for v in range(3):
            m = _miss("H", hg.information(v), _drop(c["ref_H"], d, v))
            worst = max(worst, (m, name))
            print(f"H {name} fixed {'aij'[v]}: miss {m:.2e}")
            if not m <= DEVICE["H"]:
                bad.append((name, "aij"[v], m))
    print(f"worst {worst[0]:.2e} ({worst[1]}), bound {DEVICE['H']:.2e}")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("d", [6, 3])
def test_device_lm_recovers_the_ring_from_a_far_start(d, solver_ctx):
    """Gradient sign and pose update against the TRUTH: a noise-free ring of 8 with two chords whose absolute orientations
    lie in all four extraction branches (SE2: headings on both sides of +-pi), measurements from the reference's between,
    start 0.3 rad and 0.2 m away: chi2 from > 1 to < 1e-16, the poses equal the truth to 1e-9 up to the quaternion's sign."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    hip_ctx, solver = solver_ctx
    p = "ring3_" if d == 6 else "ring2_"
    hg = GraphWrapperHIP.from_dict(_ring(d, FX[p + "start"]), ctx=hip_ctx)
    st = hg.optimize(50, 0)
    print(f"d = {d}: chi2 {st['chi2_initial']:.6g} -> {st['chi2_final']:.3g} in {st['iterations']} iterations / {st['trials']} solves")
    assert st["solver"] == solver
    assert st["chi2_initial"] > 1.0 and st["chi2_final"] < 1e-16, st
    ids, poses = hg.vertices()
    assert np.array_equal(ids, np.arange(8))
    assert _same_poses(d, poses, FX[p + "truth"], 1e-9)
    if d == 6:
        assert np.abs(np.linalg.norm(poses[:, 3:], axis=1) - 1).max() < 1e-14 and (poses[:, 6] >= 0).all()
    else:
        assert (poses[:, 2] >= -np.pi).all() and (poses[:, 2] < np.pi).all()


@pytest.mark.gpu
@pytest.mark.parametrize("turn", [0, 1, 2])
def test_device_lm_matches_oracle_with_a_vertex_turned_by_150_degrees(turn, solver_ctx):
    """The same ring at the truth but for one vertex turned by 150 degrees about x, y, z: the INITIAL errors of its edges lie
    in the tr <= 0 branches. Device against oracle with the bounds of test_device_lm_matches_oracle, the same number of
    iterations and solves, and a decrease.
    The graph is noise-free, so LM ends on chi2 ~ 1e-28 (from the 18th iteration on), where accepting or rejecting a step
    is decided by the rounding of chi2 itself: there the two implementations take 21-25 iterations and 38-48 solves each,
    with every figure inside its bound. The counts are therefore compared after LM_STEPS = 12 iterations (chi2 ~ 1e-10, ten
    orders above that floor, all rejected trials of the far start included), the final state after the remaining ones."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    hip_ctx, solver = solver_ctx
    g = _ring(6, FX["ring3_turned"][turn])
    assert {_branch(_error_quat({"xi": g["poses"][a], "xj": g["poses"][b], "z": g["edge_data"][e, :7]}))[0]
            for e, (a, b) in enumerate(g["edge_ij"]) if 3 in (a, b)} <= {"x", "y", "z"}
    og = oracle_lib.OracleGraph.from_dict(g)
    hg = GraphWrapperHIP.from_dict(g, ctx=hip_ctx)

    def same_state():
        ph, po = hg.vertices()[1], og.vertices()[1]
        sign = np.sign(np.sum(ph[:, 3:] * po[:, 3:], axis=1))[:, None]
        ph = np.concatenate([ph[:, :3], ph[:, 3:] * sign], axis=1)
        return np.abs(ph - po).max() <= 1e-7 * max(1.0, np.abs(po).max())

    ref, got = og.optimize(LM_STEPS, 0), hg.optimize(LM_STEPS, 0)
    print(f"turn about {'xyz'[turn]}: chi2 {got['chi2_initial']:.6g} -> {got['chi2_final']:.6g} in {got['iterations']} / {got['trials']} "
          f"(oracle {ref['chi2_final']:.6g} in {ref['iterations']:.0f} / {ref['trials']:.0f})")
    assert got["solver"] == solver
    assert got["chi2_initial"] == pytest.approx(ref["chi2_initial"], rel=1e-9)
    assert got["chi2_final"] == pytest.approx(ref["chi2_final"], rel=1e-7, abs=1e-12)
    assert got["chi2_final"] < got["chi2_initial"]
    assert (got["iterations"], got["trials"]) == (int(ref["iterations"]), int(ref["trials"]))
    assert int(ref["trials"]) > LM_STEPS        # the far start does cost rejected trials
    assert same_state()
    ref2, got2 = og.optimize(50, 0), hg.optimize(50, 0)
    print(f"    then chi2 {got2['chi2_final']:.6g} in {got2['iterations']} / {got2['trials']} (oracle {ref2['chi2_final']:.6g} in "
          f"{ref2['iterations']:.0f} / {ref2['trials']:.0f})")
    assert got2["chi2_final"] == pytest.approx(ref2["chi2_final"], rel=1e-7, abs=1e-12)
    assert got2["chi2_final"] < got["chi2_initial"]
    assert same_state()


@pytest.mark.gpu
def test_device_kld_estimate_difference_at_large_rotations(solver_ctx):
    """pose_diff_kernel: baseline and `other` are the same 6-vertex graph, other's estimates displaced by rotations in every
    branch. kullbackLeiblerDivergence (src/utils.cpp:70-97, as the oracle's kullback_leibler restates it):
    mahalanobis = diff^T infox diff with infox = other->information() and diff = estimateDifference(other)
    (src/graph_wrapper_g2o.cpp:544-575). Rebuilt in numpy from the reference diff and the device's information() of `other`
    (pinned by test_device_information_of_every_case), and compared with the oracle's term."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    hip_ctx, solver = solver_ctx
    gb = {"pose_dim": 6, "ids": np.arange(6, dtype=np.int32), "poses": FX["kld_base"], "edge_ij": FX["kld_ij"], "edge_data": FX["kld_data"]}
    go = dict(gb, poses=FX["kld_other"])
    base, other = GraphWrapperHIP.from_dict(gb, ctx=hip_ctx), GraphWrapperHIP.from_dict(go, ctx=hip_ctx)
    base.kullbackLeibler(other, 0)
    got = base.last_kld_terms["mahalanobis"]
    diff = FX["kld_ref_diff"].reshape(-1)
    Ho = other.information(0)
    want = float(diff @ Ho @ diff)
    ref = oracle_lib.OracleGraph.from_dict(gb).kullback_leibler(oracle_lib.OracleGraph.from_dict(go), 0)
    print(f"mahalanobis: device {got:.17g}, diff^T H diff {want:.17g}, oracle {ref['mahalanobis']:.17g}")
    assert want > 1.0
    assert abs(got - want) <= util.RTOL * want
    assert abs(got - ref["mahalanobis"]) <= util.RTOL * want


def _star_graph():
    P, om, B = FX["star_poses"], FX["star_omega"], FX["star_ref_between"]
    ij = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (3, 4)]
    data = [np.concatenate([B[a, b], om[e]]) for e, (a, b) in enumerate(ij)]
    return {"pose_dim": 6, "ids": np.arange(5, dtype=np.int32), "poses": P, "edge_ij": np.array(ij, np.int32), "edge_data": np.array(data)}


def _check_star_edges(edges):
    """Every measurement of the new edges against the reference: pose-pose edges (alone or inside a correlated edge) carry
    between(Xa, Xb) as a unit quaternion with w >= 0, n-ary GLC edges the reparametrisation (first pose absolute, the
    others relative to it, compact quaternions of w >= 0). Returns the worst miss."""
    P, B = FX["star_poses"], FX["star_ref_between"]
    worst, n = 0.0, 0
    for kind, ids, data in util.edge_list(edges):
        if kind == abi.EDGE_BINARY:
            meas = [(ids[0], ids[1], data[:7])]
        elif kind == abi.EDGE_MULTI:
            pairs, ms, _ = util.multi_parts(6, data)
            meas = [(ids[a], ids[b], m) for (a, b), m in zip(pairs, ms)]
        else:
            meas = []
            for k, v in enumerate(ids):
                want = P[ids[0]][:6] if k == 0 else B[ids[0], v][:6]
                got = data[6 * k:6 * k + 6]
                assert (got[3:] ** 2).sum() <= 1.0
                worst = max(worst, _miss("between", got, want))
                n += 1
        for a, b, m in meas:
            assert abs(np.linalg.norm(m[3:]) - 1) < 1e-15 and m[6] >= 0, (a, b, m)
            worst = max(worst, _miss("between", m, B[a, b]))
            n += 1
    assert n > 0
    return worst


STAR_ALGORITHMS = {"nfr_tree": (abi.ALG_NFR, abi.TOPO_TREE), "glc_tree": (abi.ALG_GLC, abi.TOPO_TREE),
                   "nfr_dense": (abi.ALG_NFR, abi.TOPO_DENSE), "glc_dense": (abi.ALG_GLC, abi.TOPO_DENSE)}


def _run_star(ctx, alg):
    """Remove the root of the star on the device and in the oracle -> (worst measurement miss, worst edge miss vs oracle)"""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g = _star_graph()
    a, t = STAR_ALGORITHMS[alg]
    opts = abi.make_options(6, a, t)
    which = np.array([0], np.int32)
    hg = GraphWrapperHIP.from_dict(g, ctx=ctx, useGLC=(a == abi.ALG_GLC))
    st = hg.marginalizeNoOptimize(which, opts)
    assert st["n_bad_status"] == 0 and st["n_removed"] == 1, st
    og = oracle_lib.OracleGraph.from_dict(g)
    assert og.marginalize(which, opts) == 0
    return _check_star_edges(hg.edges()), util.compare_edge_sets(6, og.edges(), hg.edges(), rtol=util.RTOL)


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ["nfr_tree", "glc_tree", "nfr_dense"])
def test_device_new_edge_measurements_at_large_relative_rotations(alg, hip_ctx):
    """Measurement from state (setMeasurementFromState, R_to_quat(Z) of the new-edge sites; NFR Dense through the
    interior-point kernel's own): an SE3 star whose neighbours' relative rotations lie in every branch, root removed."""
    worst, vs_oracle = _run_star(hip_ctx, alg)
    print(f"{alg}: measurements against the reference {worst:.2e} (bound {DEVICE['between']:.2e}), edges against the oracle {vs_oracle:.2e}")
    assert worst <= DEVICE["between"]


FORCED = r'''
import os, sys
os.environ["SPG_FORCE_BIG"] = "1"
sys.path.insert(0, sys.argv[1])
from sparsifyposegraph_amd.lib import Context
from tests import test_device_geometry as t
ctx = Context(0)
ctx.profile(True)
worst, vs_oracle = t._run_star(ctx, "glc_dense")
big = ctx.profile_read_big()
assert big["blankets"] == 1, big
assert worst <= t.DEVICE["between"], worst
print(f"forced ok: measurements against the reference {worst:.2e}, edges against the oracle {vs_oracle:.2e}")
'''


@pytest.mark.gpu
def test_device_new_edge_measurements_through_the_large_blanket_pipeline(tmp_path):
    """The same star through big_reparam_kernel: GLC Dense with every blanket forced into the dense HBM pipeline
    (SPG_FORCE_BIG=1, read once per process: own process, as tests/test_big_blankets.py does)."""
    script = tmp_path / "forced_star.py"
    script.write_text(FORCED)
    out = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "forced ok" in out.stdout
    print(out.stdout)
