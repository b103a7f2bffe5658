"""Factor descent for the NFR patterns without a closed form (SPG_FLAG_NFR_FACTOR_DESCENT, include/spg.h).
CPU: the numpy restatement tests/factor_descent_ref.py against the properties of the algorithm (monotone, positive
definite), against an independent BFGS solution, the oracle's interior point and the Chow-Liu tree, on the oracle's
Lambda_t and patterns; the planner under the flag (tests/cpp/factor_descent_plan_demo.cpp). GPU: csrc/spg_nfr_fd.inc
against the restatement at a fixed cycle count, its converged result against the oracle, the paths the flag must not
touch, a blanket beyond the interior point's Newton-system limit, a whole graph, the C++ facade."""
import functools
import os
import subprocess

import numpy as np
import pytest

from sparsifyposegraph_amd import abi, g2o_io
from tests import factor_descent_ref as fdr
from tests import oracle_lib, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")


def _opts(d, topo, chord=1.0, fd=False):
    o = abi.make_options(d, abi.ALG_NFR, topo, factor_descent=fd)
    o.chord_ratio = chord
    return o


def _blocks(d, res, b):
    """[(original vertex ids, X)] of blanket b of a marginalize_batch result"""
    ps, il = abi.pose_stride(d), d * (d + 1) // 2
    out = []
    for e in range(res["new_edge_off"][b], res["new_edge_off"][b + 1]):
        v = res["new_edge_vert"][res["new_edge_vert_off"][e]:res["new_edge_vert_off"][e + 1]]
        data = res["new_edge_data"][res["new_edge_data_off"][e]:res["new_edge_data_off"][e + 1]]
        X = np.zeros((d, d))
        X[np.triu_indices(d)] = data[ps:ps + il]
        out.append((tuple(int(x) for x in v), X + np.triu(X, 1).T))
    return out


def _blanket_inputs(d, batch, res, b):
    """(Lambda_t, pattern as local kept indices, kept poses) of blanket b: the inputs of the restatement"""
    v0, v1, m = batch["vert_off"][b], batch["vert_off"][b + 1], batch["n_remove"][b]
    n = d * (v1 - v0 - m)
    lam = res["target_info"][res["target_info_off"][b]:res["target_info_off"][b] + n * n].reshape(n, n)
    local = {int(v): i - m for i, v in enumerate(np.asarray(batch["vert_id"])[v0:v1])}
    pairs = [(local[a], local[c]) for (a, c), _ in _blocks(d, res, b)]
    poses = np.asarray(batch["pose"]).reshape(-1, abi.pose_stride(d))[v0 + m:v1]
    return lam, pairs, poses


def _ip_blankets(batch, res):
    """indices of the blankets whose pattern has more than k - 1 edges: the interior point's / factor descent's"""
    ne = np.diff(res["new_edge_off"])
    k = np.diff(batch["vert_off"]) - batch["n_remove"]
    return np.nonzero(ne > np.maximum(k - 1, 0))[0]


@functools.lru_cache(maxsize=None)
def _first_round(case, topo, chord):
    """first-round batch of a golden case with the oracle's interior-point and Tree results"""
    g, which, opts, *_ = util.load_golden(case)
    d = opts.pose_dim
    batch, roots = util.first_round_batch(g, which, _opts(d, topo, chord))
    oracle = oracle_lib.lib()
    ref = abi.marginalize_batch(oracle, None, _opts(d, topo, chord), batch)
    tree = abi.marginalize_batch(oracle, None, _opts(d, abi.TOPO_TREE), batch)
    assert (ref["status"] == 0).all() and (tree["status"] == 0).all()
    return d, batch, ref, tree, _ip_blankets(batch, ref)


# ------------------------------------------------------------------------------------------------------ CPU
CPU_CASES = [("manhattan_nfr_tree", abi.TOPO_DENSE, 1.0), ("intel_nfr_tree_sp3", abi.TOPO_SUBGRAPH, 0.4)]
N_CPU = 16     # blankets per case, the first ones of the round (SE2, k = 3 .. 16)


@functools.lru_cache(maxsize=None)
def _converged(case, topo, chord):
    d, batch, ref, tree, ip = _first_round(case, topo, chord)
    assert len(ip) >= N_CPU
    return [(int(b), fdr.run(d, *_blanket_inputs(d, batch, ref, b))) for b in ip[:N_CPU]]


@pytest.mark.parametrize("case,topo,chord", CPU_CASES)
def test_restatement_is_monotone_and_positive_definite(case, topo, chord):
    """The KLD never rises from one cycle to the next (1e-13 max(1, KLD)); every final information is positive definite;
    the default stop rule ends every run far below max_cycles."""
    worst_rise, most = -np.inf, 0
    for b, r in _converged(case, topo, chord):
        assert r["status"] == fdr.ST_OK and not r["hit_max"] and r["cycles"] >= 1
        tr = np.array(r["trace"])
        rise = np.diff(tr) / np.maximum(1.0, np.abs(tr[1:]))
        worst_rise, most = max(worst_rise, rise.max()), max(most, r["cycles"])
        assert (rise <= 1e-13).all(), (b, rise.max())
        for X in r["X"]:
            assert np.linalg.eigvalsh(X).min() > 0, b
    print(f"{case} topo={topo}: {N_CPU} blankets, largest KLD rise {worst_rise:.1e}, at most {most} cycles")


@pytest.mark.parametrize("case,topo,chord", CPU_CASES)
def test_restatement_against_interior_point_and_tree(case, topo, chord):
    """Final KLD <= the oracle's interior-point KLD + 1e-7, the oracle above it by at most the barrier bias 5e-6 (the bound
    tests/test_interior_point.py uses), and <= the oracle's Tree KLD of the same blanket + 1e-9."""
    d, batch, ref, tree, ip = _first_round(case, topo, chord)
    gaps = []
    for b, r in _converged(case, topo, chord):
        gap = ref["kld"][b] - r["kld"]
        gaps.append(gap)
        assert r["kld"] <= ref["kld"][b] + 1e-7, (b, r["kld"], ref["kld"][b])
        assert -1e-7 <= gap <= 5e-6, (b, gap)
        assert r["kld"] <= tree["kld"][b] + 1e-9, (b, r["kld"], tree["kld"][b])
    print(f"{case} topo={topo}: interior point minus factor descent {min(gaps):.2e} .. {max(gaps):.2e}")


def test_restatement_against_bfgs():
    """The optimum of the parametrisation of test_oracle_interior_point_finds_the_minimiser (X_e = L_e L_e^T, BFGS on the
    Cholesky parameters, scipy) over the restatement's own J U and S: final KLD <= that optimum + 1e-7."""
    from scipy.optimize import minimize
    case, topo, chord = CPU_CASES[0]
    d, batch, ref, tree, ip = _first_round(case, topo, chord)
    tri = np.tril_indices(d)
    done = 0
    for b, r in _converged(case, topo, chord):
        lam, pairs, poses = _blanket_inputs(d, batch, ref, b)
        if len(pairs) < 3 or done >= 4:
            continue
        Js = fdr.jacobians(d, poses, pairs)
        U, S, _ = fdr.spectrum(d, lam, Js)
        Jt = [J @ U for J in Js]
        rr = U.shape[1]

        def f(p):
            M = np.zeros((rr, rr))
            for e in range(len(Jt)):
                L = np.zeros((d, d))
                L[tri] = p[e * len(tri[0]):(e + 1) * len(tri[0])]
                M += Jt[e].T @ (L @ L.T) @ Jt[e]
            sign, ld = np.linalg.slogdet(M)
            if sign <= 0:
                return 1e30
            return 0.5 * (np.sum(np.diag(M) * S) - ld - np.log(S).sum() - rr)

        best = minimize(f, np.concatenate([np.eye(d)[tri]] * len(Jt)), method="BFGS", options={"gtol": 1e-9, "maxiter": 4000})
        print(f"blanket {b}: E = {len(pairs)}, factor descent {r['kld']:.12g} in {r['cycles']} cycles, BFGS {best.fun:.12g}")
        assert r["kld"] <= best.fun + 1e-7, (b, r["kld"], best.fun)
        done += 1
    assert done >= 2


def test_abi_names():
    assert abi.FLAG_NFR_FACTOR_DESCENT == 8 and abi.INFO_FD_MAX_CYCLES == 16
    assert abi.make_options(6, factor_descent=True).flags == 8
    assert abi.make_options(6, flags=abi.FLAG_FORCE_EIG, factor_descent=True).flags == 10
    text = open(os.path.join(ROOT, "include", "spg.h")).read()
    assert "SPG_FLAG_NFR_FACTOR_DESCENT = 8" in text and "SPG_INFO_FD_MAX_CYCLES = 16" in text
    assert "int spg_ctx_set_factor_descent(spg_ctx *ctx, double rel_tol, int max_cycles);" in text


def test_setter_on_an_injected_context():
    """spg_ctx_set_factor_descent validates its arguments on every context; backends other than the HIP one ignore it."""
    ctx = oracle_lib.injected_context()
    ctx.set_factor_descent(1e-10, 50)
    ctx.set_factor_descent(0.0, 20)
    ctx.set_factor_descent()
    from sparsifyposegraph_amd.lib import SpgError
    with pytest.raises(SpgError):
        ctx.set_factor_descent(float("nan"), 5)
    with pytest.raises(SpgError):
        ctx.set_factor_descent(0.0, 40000)


def test_graph_wrapper_passes_the_flag():
    from sparsifyposegraph_amd.graph import GraphWrapperHIP, SparsityOptions
    hg = GraphWrapperHIP(ctx=oracle_lib.injected_context(), pose_dim=3)
    assert hg._flags(0) == 0
    hg.setFactorDescent()
    assert hg._flags(0) == abi.FLAG_NFR_FACTOR_DESCENT and SparsityOptions().to_abi(3, False, hg._flags(0)).flags == 8
    hg.setFactorDescent(False)
    assert hg._flags(0) == 0
    glc = GraphWrapperHIP(ctx=oracle_lib.injected_context(), pose_dim=3, useGLC=True)
    glc.setFactorDescent()
    assert glc._flags(0) == 0


def test_round_plan_under_the_flag(tmp_path):
    """A k = 23 SE3 Dense blanket (9 108 variables) plans under the flag, with a workspace smaller than the unflagged one of
    a k = 12 blanket; unflagged it is SPG_ECAPACITY with the existing message; plans the flag does not apply to are unchanged."""
    exe = str(tmp_path / "factor_descent_plan_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "factor_descent_plan_demo.cpp"),
                           "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "factor descent plan ok" in out.stdout and "FAIL" not in out.stdout


def _build_demo(tmp_path):
    exe = str(tmp_path / "factor_descent_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "factor_descent_demo.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_factor_descent_demo_compiles(tmp_path):
    out = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 2 and "usage" in out.stderr


# ------------------------------------------------------------------------------------------------------ GPU
GPU_CASES = [("manhattan_nfr_tree", abi.TOPO_DENSE, 1.0), ("sphere_nfr_tree", abi.TOPO_DENSE, 1.0), ("manhattan_nfr_tree", abi.TOPO_SUBGRAPH, 0.5)]
FIXED_CYCLES = 20


def _device_bound(d, inputs, cycles):
    """The tolerance of the device against the restatement, measured: the restatement with P recomputed after every edge
    against the one with the rank-d Woodbury update within a cycle — the largest relative difference of any X_e is the
    algorithm's own rounding sensitivity; the device gets 100 x that, never more than 1e-8. -> (restatement runs, bound, sens)"""
    runs, sens = [], 0.0
    for lam, pairs, poses in inputs:
        Js = fdr.jacobians(d, poses, pairs)
        r = fdr.run(d, lam, pairs, poses, cycles, 0.0, Js=Js)
        w = fdr.run(d, lam, pairs, poses, cycles, 0.0, woodbury=True, Js=Js)
        assert r["status"] == fdr.ST_OK and w["status"] == fdr.ST_OK
        sens = max(sens, max(np.abs(a - c).max() / np.abs(a).max() for a, c in zip(r["X"], w["X"])))
        runs.append(r)
    return runs, min(100.0 * sens, 1e-8), sens


def _against_restatement(d, batch, got, blankets, cycles, what):
    inputs = [_blanket_inputs(d, batch, got, b) for b in blankets]
    runs, bound, sens = _device_bound(d, inputs, cycles)
    worst, kerr = 0.0, 0.0
    for b, r in zip(blankets, runs):
        assert got["status"][b] == r["status"] == 0 and got["info"][b] >> 8 == cycles == r["cycles"], (b, got["status"][b], got["info"][b])
        assert got["info"][b] & abi.INFO_FD_MAX_CYCLES
        blocks = _blocks(d, got, b)
        assert len(blocks) == len(r["X"])
        for (_, Xg), Xr in zip(blocks, r["X"]):
            worst = max(worst, np.abs(Xg - Xr).max() / np.abs(Xr).max())
        kerr = max(kerr, abs(got["kld"][b] - r["kld"]) / max(1.0, abs(r["kld"])))
    print(f"{what}: {len(blankets)} blankets, {cycles} cycles: rounding sensitivity of the algorithm {sens:.2e}, device bound {bound:.2e}; "
          f"device against the restatement: informations {worst:.2e}, KLD {kerr:.2e}")
    assert worst <= bound and kerr <= bound, (worst, kerr, bound)


@pytest.fixture
def fd_ctx(hip_ctx):
    """the session's context; the factor-descent parameters are back at their defaults afterwards"""
    yield hip_ctx
    hip_ctx.set_factor_descent()


@pytest.mark.gpu
@pytest.mark.parametrize("case,topo,chord", GPU_CASES)
def test_device_fixed_cycles_match_restatement(case, topo, chord, fd_ctx):
    """rel_tol = 0, max_cycles = 20: device and numpy do the same work. First-round blankets (SE2 k = 3 .. 5 and SE3 k = 3, 4
    under Dense; Subgraph(0.5) patterns have bridges): patterns, statuses and cycle counts identical to the unflagged run /
    the restatement, informations and KLD within 100 x the measured rounding sensitivity of the algorithm (<= 1e-8).
    Measured on the MI355X: see the figures of DESIGN.md 5h-F."""
    d, batch, ref, tree, _ = _first_round(case, topo, chord)
    fd_ctx.set_factor_descent(0.0, FIXED_CYCLES)
    got = fd_ctx.marginalize_batch(_opts(d, topo, chord, fd=True), batch)
    assert np.array_equal(ref["status"], got["status"])
    assert np.array_equal(ref["new_edge_off"], got["new_edge_off"]) and np.array_equal(ref["new_edge_vert"], got["new_edge_vert"])
    ip = _ip_blankets(batch, got)
    assert len(ip) >= 10
    _against_restatement(d, batch, got, ip, FIXED_CYCLES, f"{case} topo={topo}")


@pytest.mark.gpu
@pytest.mark.parametrize("case,topo,chord", GPU_CASES)
def test_device_converged_against_oracle(case, topo, chord, fd_ctx):
    """Default settings: per blanket kld_fd <= kld_tree + 1e-9 and <= the oracle's interior-point KLD + 1e-7, every
    information positive definite, no blanket at max_cycles."""
    d, batch, ref, tree, _ = _first_round(case, topo, chord)
    fd_ctx.set_factor_descent()
    got = fd_ctx.marginalize_batch(_opts(d, topo, chord, fd=True), batch)
    assert np.array_equal(ref["status"], got["status"]) and np.array_equal(ref["new_edge_vert"], got["new_edge_vert"])
    ip = _ip_blankets(batch, got)
    assert len(ip) >= 10
    cyc = got["info"][ip] >> 8
    print(f"{case} topo={topo}: {len(ip)} blankets, cycles mean {cyc.mean():.1f} max {cyc.max()}, "
          f"interior point minus factor descent {np.min(ref['kld'][ip] - got['kld'][ip]):.2e} .. {np.max(ref['kld'][ip] - got['kld'][ip]):.2e}")
    assert not (got["info"][ip] & abi.INFO_FD_MAX_CYCLES).any() and (cyc >= 1).all()
    assert (got["kld"][ip] <= tree["kld"][ip] + 1e-9).all()
    assert (got["kld"][ip] <= ref["kld"][ip] + 1e-7).all()
    for b in ip:
        for _, X in _blocks(d, got, b):
            assert np.linalg.eigvalsh(X).min() > 0, b


def _same_bytes(a, b, keys):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _by_root(bl):
    """blanket records in the order of their roots (the order of the records is the order in which batches were committed)"""
    order = np.argsort(bl["root"], kind="stable")
    return {k: np.ascontiguousarray(v[order]) for k, v in bl.items()}


@pytest.mark.gpu
def test_tree_shaped_blankets_of_a_subgraph_run_are_untouched(fd_ctx):
    """Inside a flagged Subgraph run the blankets whose pattern is a tree are byte-identical to the unflagged run."""
    d, batch, ref, tree, _ = _first_round("manhattan_nfr_tree", abi.TOPO_SUBGRAPH, 0.5)
    plain = fd_ctx.marginalize_batch(_opts(d, abi.TOPO_SUBGRAPH, 0.5), batch)
    got = fd_ctx.marginalize_batch(_opts(d, abi.TOPO_SUBGRAPH, 0.5, fd=True), batch)
    ip = set(int(b) for b in _ip_blankets(batch, got))
    others = [b for b in range(len(got["status"])) if b not in ip]
    assert len(others) >= 10 and len(ip) >= 10
    _same_bytes(plain, got, ("status", "new_edge_off", "new_edge_vert", "new_edge_data_off", "target_info"))
    for b in others:
        e0, e1 = got["new_edge_off"][b], got["new_edge_off"][b + 1]
        lo, hi = got["new_edge_data_off"][e0], got["new_edge_data_off"][e1]
        assert plain["new_edge_data"][lo:hi].tobytes() == got["new_edge_data"][lo:hi].tobytes(), b
        assert plain["kld"][b:b + 1].tobytes() == got["kld"][b:b + 1].tobytes() and plain["info"][b] == got["info"][b], b
    assert any((plain["info"][b] >> 8) != (got["info"][b] >> 8) for b in ip)      # ... and the others did take the other solver


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sphere_nfr_tree", "sphere_cliquey_subgraph", "manhattan_glc_tree"])
def test_flag_leaves_other_patterns_untouched(case, fd_ctx):
    """Tree, CliqueySubgraph and GLC Tree graphs of the golden cases: the flagged run is byte-identical to the unflagged one —
    edges and, per root, status, info, KLD and gap. (Not the round number: NFR Tree lists go through the streaming driver,
    whose round is the doorbell a blanket happened to ride.)"""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, which, opts, *_ = util.load_golden(case)
    runs = []
    for flag in (0, abi.FLAG_NFR_FACTOR_DESCENT):
        o = abi.Options.from_buffer_copy(opts)
        o.flags |= flag
        hg = GraphWrapperHIP.from_dict(g, ctx=fd_ctx)
        st = hg.marginalizeNoOptimize(which, o)
        runs.append((hg.edges(), hg.blankets(), st))
    (ea, ba, sa), (eb, bb, sb) = runs
    assert sa["n_removed"] == sb["n_removed"] > 0 and sa["n_bad_status"] == sb["n_bad_status"]
    _same_bytes(ea, eb, ea.keys())
    _same_bytes(_by_root(ba), _by_root(bb), [k for k in ba.keys() if k != "round"])


@pytest.mark.gpu
@pytest.mark.parametrize("k,cycles", [(8, 20), (23, 30)])
def test_hub_blanket_against_restatement(k, cycles, fd_ctx):
    """The hub of an SE3 hub graph under Dense, built as the interior point's hub tests build theirs. k = 8 (28 edges): the
    buffers outgrow LDS and the cycle runs out of the L2 workspace. k = 23 (253 edges, d^2 E = 9 108): beyond the interior
    point's Newton-system limit — SPG_ECAPACITY unflagged — and at n = 138 the per-cycle factorisation and inverse run
    blocked on the matrix cores. Flagged, a fixed number of cycles: status OK, all edges positive definite, a finite KLD,
    agreement with the restatement to the measured bound."""
    from tests.test_big_blankets import _star_graph
    g = _star_graph(k, seed=5)
    batch, roots = util.first_round_batch(g, np.array([0], np.int32), _opts(6, abi.TOPO_DENSE))
    assert roots == [0]
    if 36 * k * (k - 1) // 2 > 8400:
        with pytest.raises(RuntimeError, match=f"rc={abi.ECAPACITY}"):
            fd_ctx.marginalize_batch(_opts(6, abi.TOPO_DENSE), batch)
    fd_ctx.set_factor_descent(0.0, cycles)
    got = fd_ctx.marginalize_batch(_opts(6, abi.TOPO_DENSE, fd=True), batch)
    assert got["status"][0] == 0 and got["new_edge_off"][1] == k * (k - 1) // 2 and np.isfinite(got["kld"][0])
    for _, X in _blocks(6, got, 0):
        assert np.linalg.eigvalsh(X).min() > 0
    _against_restatement(6, batch, got, [0], cycles, f"hub with {k} neighbours under Dense")


@pytest.mark.gpu
def test_whole_graph_through_the_scheduler(fd_ctx):
    """manhattan prefix of 400 poses under Subgraph(0.34), flagged (the unflagged interior-point test's case): no bad
    status, two runs byte-identical, optimize() runs, the global KLD against the baseline is finite (printed next to the
    unflagged run's: sequential sparsification does not order the two)."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, which, opts, *_ = util.load_golden("manhattan_nfr_tree")
    sub, w = util.prefix_graph(g, which, 400)
    fd_ctx.set_factor_descent()
    runs = {}
    for name, fd in (("fd", True), ("fd again", True), ("interior point", False)):
        hg = GraphWrapperHIP.from_dict(sub, ctx=fd_ctx)
        st = hg.marginalizeNoOptimize(w, _opts(3, abi.TOPO_SUBGRAPH, 0.34, fd=fd))
        assert st["n_bad_status"] == 0
        runs[name] = (hg, hg.edges(), hg.blankets(), st)
    _same_bytes(runs["fd"][1], runs["fd again"][1], runs["fd"][1].keys())
    _same_bytes(_by_root(runs["fd"][2]), _by_root(runs["fd again"][2]), runs["fd"][2].keys())
    base = GraphWrapperHIP.from_dict(sub, ctx=fd_ctx)
    gk = {name: base.kullbackLeibler(runs[name][0]) for name in ("fd", "interior point")}
    hb = runs["fd"][2]
    cyc = (hb["info"] >> 8)[(hb["info"] >> 8) > 0]
    assert len(cyc) >= 3 and not (hb["info"] & abi.INFO_FD_MAX_CYCLES).any()
    print(f"manhattan prefix, Subgraph(0.34): {len(cyc)} blankets by factor descent (cycles mean {cyc.mean():.1f} max {cyc.max()}); "
          f"kld_sum {runs['fd'][3]['kld_sum']:.9g} (interior point {runs['interior point'][3]['kld_sum']:.9g}); "
          f"global KLD {gk['fd']:.9g} (interior point {gk['interior point']:.9g})")
    assert np.isfinite(gk["fd"])
    ost = runs["fd"][0].optimize()
    assert np.isfinite(ost["chi2_final"])


@pytest.mark.gpu
def test_cpp_facade_factor_descent(tmp_path):
    path = str(tmp_path / "s200.g2o")
    g2o_io.write_g2o(path, g2o_io.synth_sphere(n_poses=200, ring=20))
    out = subprocess.run([_build_demo(tmp_path), path], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "factor descent ok" in out.stdout
