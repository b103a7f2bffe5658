"""optimize() with the preconditioned conjugate-gradient linear solver (SPG_SOLVER_PCG, csrc/spg_bsr.inc: PcgLM — g2o's
PCG solver family next to its dense and sparse Cholesky ones): block-Jacobi preconditioned CG on the block-CSR information
of tests/test_sparse_information.py. All GPU: against the Cholesky routes on the noise-free and the noisy rings of
tests/test_optimize.py and its perturbed goldens, an iteration cap of one (inexact LM steps), and that selecting PCG
changes nothing for the KLD, the covariances and the other solvers."""
import numpy as np
import pytest

from sparsifyposegraph_amd import abi, g2o_io
from tests.test_optimize import _perturbed

# chi2_final and the estimates under PCG against the sparse and the dense Cholesky. Worst relative difference measured on
# the MI355X over the graphs below: 2.02e-8, the estimates of the noisy rings against either Cholesky route
# (chi2_final there agrees to 1.8e-16; every other figure is below 1.8e-8). The bound is ten times that, inside the 1e-6
# the comparison may never exceed.
PCG_VS_CHOLESKY = 2.02e-7
assert PCG_VS_CHOLESKY <= 1e-6


def _rings(noise_free):
    """synth_sphere(120, 12) started off its ground truth, as test_oracle_lm_recovers_noise_free_poses builds it: with the
    measurements rebuilt from the ground truth (chi2 -> 0) or with the generator's noisy ones"""
    g = g2o_io.synth_sphere(120, 12)
    data = np.array(g["edge_data"], float)
    if noise_free:
        for e, (a, b) in enumerate(g["edge_ij"]):
            pa, pb = g["poses"][a], g["poses"][b]
            data[e, :3] = g2o_io.quat_rotate(g2o_io.quat_conj(pa[3:]), pb[:3] - pa[:3])
            q = g2o_io.quat_mul(g2o_io.quat_conj(pa[3:]), pb[3:])
            data[e, 3:7] = q if q[3] >= 0 else -q
    rng = np.random.default_rng(1)
    P = np.array(g["poses"], float).copy()
    P[1:, :3] += 0.05 * rng.standard_normal((len(P) - 1, 3))
    q = P[1:, 3:] + 0.01 * rng.standard_normal((len(P) - 1, 4))
    P[1:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return dict(g, edge_data=data, poses=P)


# name -> (graph, max_iter of set_pcg; 0 = the default min(n, 20000)). CG ends within n iterations in exact arithmetic only:
# the 120-pose prefix of intel is one odometry chain with few closures, its H + lambda I is ill conditioned at LM's small
# lambdas and rounding delays convergence past n = 357, so that graph runs with the cap raised.
GRAPHS = {
    "rings_noise_free": (lambda: _rings(True), 0),
    "rings_noisy": (lambda: _rings(False), 0),
    "manhattan_se2": (lambda: _perturbed("manhattan_nfr_tree", 150)[0], 0),
    "intel_se2": (lambda: _perturbed("intel_nfr_tree_sp3", 120)[0], 20000),
}


def _optimize(sub, ctx, solver):
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    ctx.set_linear_solver(solver)
    try:
        hg = GraphWrapperHIP.from_dict(sub, ctx=ctx)
        st = hg.optimize(50, int(sub["ids"][0]))
        return st, hg.vertices()[1], ctx.pcg_stats()
    finally:
        ctx.set_linear_solver(abi.SOLVER_AUTO)


def _pose_diff(a, b, d):
    if d == 6:
        sign = np.sign(np.sum(a[:, 3:] * b[:, 3:], axis=1))[:, None]
        a = np.concatenate([a[:, :3], a[:, 3:] * sign], axis=1)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAPHS))
def test_pcg_optimize_matches_the_cholesky_routes(name, hip_ctx):
    """chi2_final and the estimates under PCG against SPG_SOLVER_SPARSE and SPG_SOLVER_DENSE (the reference is the
    Cholesky route); every trial is one PCG solve, every solve converges, and in fewer than n iterations."""
    make, max_iter = GRAPHS[name]
    sub = make()
    d = sub["pose_dim"]
    hip_ctx.set_pcg(0.0, max_iter)
    try:
        got, pg, ps = _optimize(sub, hip_ctx, abi.SOLVER_PCG)
    finally:
        hip_ctx.set_pcg()
    n = got["n"]
    print(f"{name}: {ps}")
    assert got["solver"] == abi.SOLVER_PCG == 3 and n == d * (len(sub["ids"]) - 1)
    assert ps["solves"] == got["trials"] > 0 and ps["unconverged"] == 0
    assert ps["iterations"] < ps["solves"] * (max_iter or n)
    assert 0.0 <= ps["last_rel_residual"] <= 1.0001e-10
    for which in (abi.SOLVER_SPARSE, abi.SOLVER_DENSE):
        ref, pr, zs = _optimize(sub, hip_ctx, which)
        assert ref["solver"] == which and zs["solves"] == 0
        dchi = abs(got["chi2_final"] - ref["chi2_final"]) / max(abs(ref["chi2_final"]), 1e-12)
        dpos = _pose_diff(pg, pr, d)
        print(f"{name} vs solver {which}: chi2 {got['chi2_initial']:.6g} -> {got['chi2_final']:.9g} (Cholesky {ref['chi2_final']:.9g}), "
              f"rel diff chi2 {dchi:.3g}, estimates {dpos:.3g}; {got['iterations']} it / {got['trials']} solves ({ref['iterations']} / {ref['trials']}), "
              f"{ps['iterations']} CG iterations, n = {n}")
        assert got["chi2_initial"] == ref["chi2_initial"]
        assert abs(got["chi2_final"] - ref["chi2_final"]) <= PCG_VS_CHOLESKY * max(abs(ref["chi2_final"]), 1e-12)
        assert dpos <= PCG_VS_CHOLESKY
    assert got["chi2_final"] < got["chi2_initial"]


@pytest.mark.gpu
def test_one_iteration_per_solve_is_an_inexact_step_not_an_error(hip_ctx):
    """set_pcg(max_iter=1): every solve stops unconverged, its iterate is the LM step and the gain test guards it."""
    sub = GRAPHS["rings_noisy"][0]()
    hip_ctx.set_pcg(0.0, 1)
    try:
        st, _, ps = _optimize(sub, hip_ctx, abi.SOLVER_PCG)
    finally:
        hip_ctx.set_pcg()
    print(f"max_iter = 1: chi2 {st['chi2_initial']:.6g} -> {st['chi2_final']:.6g}, {ps['solves']} solves, {ps['unconverged']} unconverged")
    assert st["solver"] == abi.SOLVER_PCG
    assert ps["unconverged"] > 0 and ps["unconverged"] == ps["solves"] == st["trials"] and ps["iterations"] == ps["solves"]
    assert st["chi2_final"] <= st["chi2_initial"]


@pytest.mark.gpu
def test_selecting_pcg_changes_nothing_else(hip_ctx):
    """PCG applies to optimize() alone: the global KLD and the marginal covariances return under PCG the bits they return
    under AUTO, and a context that ran PCG in between optimises with the sparse solver to the same bits as before."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    sub, w, opts = _perturbed("manhattan_nfr_tree", 150, sigma=0.0)
    noisy = _perturbed("manhattan_nfr_tree", 150)[0]
    fid = int(sub["ids"][0])

    def others():
        base, sp = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx), GraphWrapperHIP.from_dict(sub, ctx=hip_ctx)
        sp.marginalizeNoOptimize(w, opts)
        base.kullbackLeibler(sp, fid)
        terms = {k: v for k, v in base.last_kld_terms.items() if k != "device_seconds"}
        return terms, base.marginalCovariances(fixed_id=fid)[1]

    before, pose_before, _ = _optimize(noisy, hip_ctx, abi.SOLVER_SPARSE)
    kld_auto, cov_auto = others()
    hip_ctx.set_linear_solver(abi.SOLVER_PCG)
    try:
        kld_pcg, cov_pcg = others()
    finally:
        hip_ctx.set_linear_solver(abi.SOLVER_AUTO)
    assert kld_pcg == kld_auto and kld_pcg["solver"] in (abi.SOLVER_DENSE, abi.SOLVER_SPARSE)
    assert np.array_equal(cov_pcg, cov_auto)
    assert _optimize(noisy, hip_ctx, abi.SOLVER_PCG)[0]["solver"] == abi.SOLVER_PCG
    after, pose_after, zs = _optimize(noisy, hip_ctx, abi.SOLVER_SPARSE)
    drop = ("device_seconds",)
    assert {k: v for k, v in after.items() if k not in drop} == {k: v for k, v in before.items() if k not in drop}
    assert np.array_equal(pose_after, pose_before) and zs["solves"] == 0
