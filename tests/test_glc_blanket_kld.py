"""Per-blanket KLD of GLC removals (SPG_FLAG_GLC_KLD): the device value against tests/glc_kld_ref.py and against the
oracle's NFR Tree value of the same blanket, the opt-in (edges and statuses bit-identical, NaN without the flag) and the
cases in which the value is not defined (NaN + SPG_INFO_GLC_KLD_SKIPPED).

Tolerances. The reference helper evaluates the definition in multiprecision from fp64 inputs; the oracle's NFR Tree value
of the same blanket fits the same Chow-Liu marginals and conditionals, so the two agree up to the fp64 rounding of the
oracle's chain. AGREE is that agreement as measured by test_reference_matches_nfr_tree_of_the_oracle (worst value over the
sequential runs over the 120-vertex prefixes of the fixtures, relative to max(1, |kld|): 5.90e-13, on
intel_glc_tree_10pct; 2.2e-14 on manhattan, 7.9e-14 on sphere — the test prints them); the device tests allow 8 x AGREE, as
tests/test_device_geometry.py does for its references. No root of those prefixes falls under the "not defined" rules
(NOT_DEFINED), so the device test expects no skipped bit on them.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from sparsifyposegraph_amd import abi
from tests import oracle_lib, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsifyposegraph_amd")
AGREE = 6.0e-13
DEVICE_TOL = 8 * AGREE
TREE_CASES = ["manhattan_glc_tree", "sphere_glc_tree", "intel_glc_tree_10pct"]
# roots of the fixture prefixes that fall under the "not defined" rules (recorded by the CPU self-check)
NOT_DEFINED = {"manhattan_glc_tree": [], "sphere_glc_tree": [], "intel_glc_tree_10pct": []}


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


# ------------------------------------------------------------------------------------------------ blankets
def star_batch(d, k, seed, chords=2):
    """One blanket: removed vertex 0, kept 1..k, a star of pose-pose edges plus a few chords between kept vertices.
    vert_id = local index, so the new edges' vertex ids are blanket-local."""
    from tests import geom_ref as G
    rng = np.random.default_rng(seed)
    ps = abi.pose_stride(d)
    poses = np.zeros((k + 1, ps))
    for v in range(k + 1):
        if d == 3:
            poses[v] = [rng.normal(scale=3.0), rng.normal(scale=3.0), rng.uniform(-3, 3)]
        else:
            q = rng.normal(size=4)
            poses[v] = np.concatenate([rng.normal(scale=3.0, size=3), q / np.linalg.norm(q)])
    pairs = [(0, i) for i in range(1, k + 1)] + [(i, i + 1) for i in range(1, min(chords, k - 1) + 1)]
    data = []
    for a, b in pairs:
        z = np.array(G.to_float(G.between(d, G.pose(d, poses[a]), G.pose(d, poses[b]))))
        Q, _ = np.linalg.qr(rng.normal(size=(d, d)))
        om = Q @ np.diag(rng.uniform(20.0, 400.0, size=d)) @ Q.T
        om = (om + om.T) / 2
        data.append(np.concatenate([z, om[np.triu_indices(d)]]))
    rec = len(data[0])
    ne = len(pairs)
    return {"vert_off": np.array([0, k + 1], np.int32), "n_remove": np.array([1], np.int32),
            "vert_id": np.arange(k + 1, dtype=np.int32), "pose": poses.reshape(-1),
            "edge_off": np.array([0, ne], np.int32), "edge_kind": np.zeros(ne, np.int32),
            "edge_vert_off": np.arange(0, 2 * ne + 1, 2, dtype=np.int32), "edge_vert": np.array(pairs, np.int32).reshape(-1),
            "edge_data_off": np.arange(0, rec * ne + 1, rec, dtype=np.int64), "edge_data": np.concatenate(data)}


def reference_klds(d, batch, out, blankets=None):
    """tests/glc_kld_ref.py on every blanket of a batch result: Lambda_t and the new edges are the run's own"""
    from tests import glc_kld_ref
    ps = abi.pose_stride(d)
    vals = []
    B = len(batch["n_remove"])
    for b in (range(B) if blankets is None else blankets):
        v0, v1, m = batch["vert_off"][b], batch["vert_off"][b + 1], batch["n_remove"][b]
        ids = [int(x) for x in batch["vert_id"][v0 + m:v1]]
        loc = {v: i for i, v in enumerate(ids)}
        kept = [np.asarray(batch["pose"]).reshape(-1, ps)[v0 + m + i] for i in range(len(ids))]
        n = d * len(ids)
        lam = out["target_info"][out["target_info_off"][b]:out["target_info_off"][b + 1]].reshape(n, n)
        edges = []
        for e in range(out["new_edge_off"][b], out["new_edge_off"][b + 1]):
            vl = [loc[int(x)] for x in out["new_edge_vert"][out["new_edge_vert_off"][e]:out["new_edge_vert_off"][e + 1]]]
            edges.append((vl, out["new_edge_data"][out["new_edge_data_off"][e]:out["new_edge_data_off"][e + 1]]))
        vals.append(glc_kld_ref.blanket_kld(d, kept, lam, edges))
    return vals


def glc(d, topo, flag):
    return abi.make_options(d, abi.ALG_GLC, topo, glc_kld=flag)


PREFIX = 120    # vertices of the fixture prefixes, on the CPU and on the device


def graph_blanket(d, og, root):
    """The blanket of `root` in the current state of an OracleGraph as a one-blanket batch: root first, its neighbours in
    ascending id, every edge (pose-pose or GLC) with all endpoints among them, in graph order."""
    ids, poses = og.vertices()
    pos = {int(v): i for i, v in enumerate(ids)}
    el = util.edge_list(og.edges())
    nb = {root}
    for _, vs, _ in el:
        if root in vs:
            nb.update(vs)
    order = [root] + sorted(nb - {root})
    loc = {v: i for i, v in enumerate(order)}
    es = [e for e in el if all(v in loc for v in e[1])]
    evo, edo = [0], [0]
    for _, vs, data in es:
        evo.append(evo[-1] + len(vs))
        edo.append(edo[-1] + len(data))
    return {"vert_off": np.array([0, len(order)], np.int32), "n_remove": np.array([1], np.int32),
            "vert_id": np.array(order, np.int32), "pose": np.concatenate([poses[pos[v]] for v in order]),
            "edge_off": np.array([0, len(es)], np.int32), "edge_kind": np.array([e[0] for e in es], np.int32),
            "edge_vert_off": np.array(evo, np.int32), "edge_vert": np.array([loc[v] for e in es for v in e[1]], np.int32),
            "edge_data_off": np.array(edo, np.int64), "edge_data": np.concatenate([e[2] for e in es]) if es else np.zeros(0)}


def sequential_reference(d, sub, w, oracle):
    """The oracle's sequential GLC Tree over the removal list `w`, one removal at a time: root -> (reference kld of the
    edges it emits, None) or (None, why it is not defined); roots with fewer than two kept vertices -> (None, "k < 2")."""
    og = oracle_lib.OracleGraph.from_dict(sub)
    opts = glc(d, abi.TOPO_TREE, False)
    out = {}
    for root in (int(v) for v in w):
        batch = graph_blanket(d, og, root)
        if len(batch["vert_id"]) - 1 < 2:
            out[root] = (None, "k < 2")
        else:
            res = abi.marginalize_batch(oracle, None, opts, batch)
            assert res["status"][0] == 0
            out[root], = reference_klds(d, batch, res)
        assert og.marginalize(np.array([root], np.int32), opts) == 0
    return out


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case", TREE_CASES)
def test_reference_matches_nfr_tree_of_the_oracle(case, oracle):
    """The helper's KLD of the oracle's GLC Tree edges equals the oracle's NFR Tree per-blanket kld for the same root, over
    the oracle's sequential runs of both on the fixture prefix the device test uses (later blankets hold the edges earlier
    removals emitted: GLC edges in one run, pose-pose edges in the other). Records the roots that fall under the "not
    defined" rules: none; roots with fewer than two kept vertices have no value in either run."""
    g, which, opts, _, _, _ = util.load_golden(case)
    d = g["pose_dim"]
    sub, w = util.prefix_graph(g, which, PREFIX)
    ref = sequential_reference(d, sub, w, oracle)
    og = oracle_lib.OracleGraph.from_dict(sub)
    assert og.marginalize(w, abi.make_options(d, abi.ALG_NFR, abi.TOPO_TREE)) == 0
    ob = og.blankets()
    assert (ob["status"] == 0).all() and sorted(int(r) for r in ob["root"]) == sorted(ref)
    worst, undefined = 0.0, []
    for r, k, v in zip(ob["root"], ob["k"], ob["kld"]):
        val, why = ref[int(r)]
        if k < 2:
            assert why == "k < 2" and np.isnan(v)
        elif why is not None:
            undefined.append((int(r), why))
        else:
            worst = max(worst, _rel(val, v))
    print(f"{case}: {len(w)} removals, helper against the oracle's NFR Tree kld: worst {worst:.2e}; not defined: {undefined}")
    assert undefined == NOT_DEFINED[case]
    assert worst <= AGREE


@pytest.mark.parametrize("d", [3, 6])
def test_reference_vanishes_where_glc_is_exact(d, oracle):
    """k = 2: the tree is the whole target; GLC Dense: (W G)^T (W G) = Lambda_t on a full-rank target. Both give 0 up to the
    rounding of the oracle's fp64 edges. The helper itself is multiprecision: what is left is the fp64 rounding of W and
    Lambda_t in the oracle's output, a sum of rounding errors whose size and sign change with the compiler and the CPU the
    oracle was built for. Measured 6.7e-14 at worst on these stars; the factor 8 (the convention of
    tests/test_device_geometry.py) covers other builds of the oracle, not another helper."""
    for k, topo in ((2, abi.TOPO_TREE), (4, abi.TOPO_DENSE)):
        batch = star_batch(d, k, seed=11 + k)
        out = abi.marginalize_batch(oracle, None, glc(d, topo, False), batch)
        assert out["status"][0] == 0
        (val, why), = reference_klds(d, batch, out)
        assert why is None
        print(f"d={d} k={k} topology={topo}: reference kld {val:.2e}")
        assert abs(val) <= 8 * 6.8e-14


def test_flag_plumbing():
    assert abi.FLAG_GLC_KLD == 4 and abi.INFO_GLC_KLD_SKIPPED == 8
    assert C.sizeof(abi.Options) == 32
    assert abi.make_options(6, abi.ALG_GLC, glc_kld=True).flags == 4
    assert abi.make_options(6, abi.ALG_GLC, flags=abi.FLAG_FORCE_EIG, glc_kld=True).flags == 6
    assert abi.make_options(6, abi.ALG_GLC).flags == 0
    with open(os.path.join(ROOT, "include", "spg.h")) as f:
        text = f.read()
    assert "SPG_FLAG_GLC_KLD = 4" in text and "SPG_INFO_GLC_KLD_SKIPPED = 8" in text


def test_injected_backend_ignores_the_flag():
    """(the oracle has no GLC LogdetFunction either: with the flag set kld stays NaN, edges unchanged, no skipped bit)"""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, which, opts, _, _, _ = util.load_golden("manhattan_glc_tree")
    sub, w = util.prefix_graph(g, which, 60)
    res = []
    for flag in (False, True):
        ctx = oracle_lib.injected_context()
        hg = GraphWrapperHIP.from_dict(sub, ctx=ctx, useGLC=True)
        st = hg.marginalizeNoOptimize(w, glc(3, abi.TOPO_TREE, flag))
        res.append((st, hg.blankets(), hg.edges()))
    (s0, b0, e0), (s1, b1, e1) = res
    assert np.isnan(b1["kld"]).all() and s1["kld_sum"] == 0.0
    assert np.array_equal(b0["info"], b1["info"]) and np.array_equal(b0["status"], b1["status"])
    for key in e0:
        assert np.array_equal(e0[key], e1[key]), key


def test_wrapper_setter():
    from sparsifyposegraph_amd.graph import GraphWrapperHIP, SparsityOptions
    ctx = oracle_lib.injected_context()
    hg = GraphWrapperHIP(ctx=ctx, pose_dim=3, useGLC=True)
    assert hg._flags(0) == 0
    hg.setGlcBlanketKld(True)
    assert hg._flags(0) == abi.FLAG_GLC_KLD and SparsityOptions().to_abi(3, True, hg._flags(0)).flags == 4
    nfr = GraphWrapperHIP(ctx=ctx, pose_dim=3, useGLC=False)
    nfr.setGlcBlanketKld(True)
    assert nfr._flags(0) == 0


# ------------------------------------------------------------------------------------------------ GPU
# (compiled against the planner header like tests/cpp/plan_demo.cpp, the planner's test hook; no device involved)
PLAN_CPP = r'''
// Where the round planner (csrc/spg_round_plan.hpp) sends single GLC blankets: for every "D topology k" triple on the
// command line one output line "D topology k NT gws big", and first the lines "gws6 K" and "gws3 K" with the smallest k at
// which an SE3 / SE2 GLC Tree blanket no longer fits the largest LDS bin (spg_blanket_layout.hpp), i.e. takes the
// workspace variant.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "spg_round_plan.hpp"

using namespace spg;

static int route(int D, int topo, int k, int *nt, int *gws, int *big) {
    spg_options o{};
    o.pose_dim = D; o.algorithm = SPG_ALG_GLC; o.topology = topo; o.lin_point = SPG_LIN_GLOBAL; o.include_intra_clique = 1;
    o.flags = SPG_FLAG_GLC_KLD; o.chord_ratio = 1.0;
    spg_blanket_desc bd{};
    bd.n_vert = k + 1; bd.n_remove = 1; bd.n_edge = k; bd.n_new_max = k; bd.n_new_vert_max = 2 * k; bd.tinfo_off = -1;
    std::vector<int64_t> vpo(k + 1, 0);
    std::vector<spg_edge_ref> er(k);
    std::vector<int32_t> ev;
    for (int v = 1; v <= k; v++) {
        er[v - 1] = spg_edge_ref{0, D == 6 ? 28 : 9, SPG_EDGE_BINARY, (int32_t)ev.size(), 2};
        ev.push_back(0); ev.push_back(v);
    }
    spg_round_desc rd{};
    rd.opts = &o; rd.n_blankets = rd.count = 1; rd.blankets = &bd; rd.vert_pose_off = vpo.data(); rd.edges = er.data(); rd.edge_vert = ev.data();
    rd.n_vert_total = k + 1; rd.n_edge_total = k; rd.n_edge_vert_total = (int64_t)ev.size(); rd.mail_len = 64; rd.tag = 1;
    PlanConfig cfg;
    RoundPlan P;
    char err[256] = {0};
    const int rc = plan_round(&rd, cfg, WorkerState{1, 0, false}, P, err, sizeof err);
    if (rc || P.to_worker) return rc ? rc : -100;
    *big = (int)P.big_list.size();
    *nt = 0; *gws = 0;
    for (const PlanBin &B : P.bins) if (!B.list.empty()) { *nt = B.variant.NT; *gws = B.variant.gws ? 1 : 0; }
    return 0;
}

int main(int argc, char **argv) {
    const PlanConfig cfg;
    for (int D : {6, 3}) {
        int kg = -1;
        for (int k = 2; k < 200 && kg < 0; k++) {
            const Layout L = make_layout(D, 256, k, 1, SPG_ALG_GLC, SPG_TOPO_TREE, 0);
            if ((size_t)(L.small_doubles + L.mat_doubles) * 8 > (size_t)cfg.lds_limit) kg = k;
        }
        printf("gws%d %d\n", D, kg);
    }
    for (int i = 1; i + 2 < argc; i += 3) {
        const int D = atoi(argv[i]), topo = atoi(argv[i + 1]), k = atoi(argv[i + 2]);
        int nt = 0, gws = 0, big = 0;
        if (int rc = route(D, topo, k, &nt, &gws, &big)) { printf("error %d\n", rc); return 1; }
        printf("%d %d %d %d %d %d\n", D, topo, k, nt, gws, big);
    }
    return 0;
}
'''


def planned_routes(tmp_path, shapes):
    """(D, topology, k) -> (NT, workspace variant?, large-blanket list) from the round planner, and {D: first k that takes
    the workspace variant}"""
    src, exe = tmp_path / "glc_kld_plan.cpp", str(tmp_path / "glc_kld_plan")
    src.write_text(PLAN_CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"), "-o", exe, str(src),
                           "-L" + PKG, "-lspg_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe] + [str(x) for s in shapes for x in s], capture_output=True, text=True, check=True).stdout.split("\n")
    kg = {6: int(out[0].split()[1]), 3: int(out[1].split()[1])}
    routes = {}
    for line in out[2:]:
        if line.strip():
            D, topo, k, nt, gws, big = (int(x) for x in line.split())
            routes[(D, topo, k)] = (nt, bool(gws), big)
    return kg, routes


# smallest SE3 / SE2 GLC Tree blankets beyond the largest LDS bin (asserted against spg_blanket_layout.hpp below)
STAR_GWS_K = 10
STAR_GWS_K2 = 22
STARS = [(3, 4), (6, 4), (6, 5), (6, STAR_GWS_K), (3, STAR_GWS_K2)]


def test_planner_routes_of_the_device_shapes(tmp_path):
    """Which kernel variant each shape of test_device_star reaches (CPU: pure planner arithmetic)"""
    T, Dn = abi.TOPO_TREE, abi.TOPO_DENSE
    shapes = [(d, t, k) for d, k in STARS for t in (T, Dn)] + [(6, T, STAR_GWS_K - 1), (3, T, STAR_GWS_K2 - 1)]
    kg, routes = planned_routes(tmp_path, shapes)
    assert kg == {6: STAR_GWS_K, 3: STAR_GWS_K2}
    for d, t, k in shapes:
        if (d, k) in ((6, STAR_GWS_K), (3, STAR_GWS_K2)):
            assert routes[(d, t, k)] == (256, True, 0), ((d, t, k), routes[(d, t, k)])     # four wavefronts, tiles in the workspace
        else:
            assert routes[(d, t, k)] == (64, False, 0), ((d, t, k), routes[(d, t, k)])     # one wavefront, tiles in LDS


@pytest.mark.gpu
@pytest.mark.parametrize("topo", [abi.TOPO_TREE, abi.TOPO_DENSE], ids=["tree", "dense"])
@pytest.mark.parametrize("d,k", STARS)
def test_device_star(d, k, topo, hip_ctx):
    """Single-blanket stars with chords, flag set: SE2 n = 12, SE3 n = 24 (register routines), n = 30 (LDS-cooperative
    routines) and the first SE3 and SE2 blankets whose tiles live in the workspace. Device kld against the helper; edges and status
    bit-identical to the unflagged run, whose kld is NaN."""
    batch = star_batch(d, k, seed=100 * d + k)
    off = hip_ctx.marginalize_batch(glc(d, topo, False), batch)
    on = hip_ctx.marginalize_batch(glc(d, topo, True), batch)
    assert off["status"][0] == 0 and np.isnan(off["kld"][0]) and off["info"][0] == 0
    for key in ("status", "new_edge_off", "new_edge_kind", "new_edge_vert_off", "new_edge_vert", "new_edge_data_off", "new_edge_data", "target_info"):
        assert np.array_equal(off[key], on[key]), key
    (val, why), = reference_klds(d, batch, on)
    assert why is None
    print(f"d={d} k={k} topology={topo}: device {on['kld'][0]:.12e} reference {val:.12e} info {on['info'][0]}")
    assert on["info"][0] == 0
    assert np.isfinite(on["kld"][0])
    assert _rel(on["kld"][0], val) <= DEVICE_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("case", TREE_CASES)
def test_device_fixture_prefix(case, hip_ctx):
    """A prefix of each GLC Tree fixture through the round driver, flag set: edges, statuses and info bit-identical to an
    unflagged device run (the skipped bit aside), the skipped bit on exactly the roots the CPU self-check recorded (none), every
    kld finite (NaN exactly on blankets with fewer than two kept vertices, as in the NFR branch) and equal to the oracle's NFR Tree value of the same root, kld_sum their sum."""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, which, opts, _, _, _ = util.load_golden(case)
    d = g["pose_dim"]
    sub, w = util.prefix_graph(g, which, PREFIX)
    runs = []
    for flag in (False, True):
        hg = GraphWrapperHIP.from_dict(sub, ctx=hip_ctx, useGLC=True)
        st = hg.marginalizeNoOptimize(w, glc(d, abi.TOPO_TREE, flag))
        assert st["n_bad_status"] == 0
        runs.append((st, hg.blankets(), hg.edges()))
    (s0, b0, e0), (s1, b1, e1) = runs
    for key in e0:
        assert np.array_equal(e0[key], e1[key]), key
    assert np.array_equal(b0["root"], b1["root"]) and np.array_equal(b0["status"], b1["status"])
    assert np.isnan(b0["kld"]).all() and s0["kld_sum"] == 0.0
    og = oracle_lib.OracleGraph.from_dict(sub)
    assert og.marginalize(w, abi.make_options(d, abi.ALG_NFR, abi.TOPO_TREE)) == 0
    ob = og.blankets()
    want = {int(r): (float(v), int(k)) for r, v, k in zip(ob["root"], ob["kld"], ob["k"])}
    skipped = [int(r) for r, inf in zip(b1["root"], b1["info"]) if inf & abi.INFO_GLC_KLD_SKIPPED]
    assert skipped == [r for r, _ in NOT_DEFINED[case]]
    worst, total = 0.0, 0.0
    for r, v in zip(b1["root"], b1["kld"]):
        ref, k = want[int(r)]
        # NaN exactly where fewer than two vertices are kept (nothing to compare, as in the NFR branch)
        assert np.isfinite(v) == (k >= 2 and int(r) not in skipped), (int(r), k, v)
        if np.isfinite(v):
            worst = max(worst, _rel(v, ref))
            total += v
    assert np.array_equal(b0["info"], b1["info"] & ~abi.INFO_GLC_KLD_SKIPPED)
    print(f"{case}: {len(w)} removals, device GLC kld against the oracle's NFR Tree kld: worst {worst:.2e}, kld_sum {s1['kld_sum']:.9g}")
    assert worst <= DEVICE_TOL
    assert abs(s1["kld_sum"] - total) <= 1e-12 * max(1.0, abs(total))


def deficient_graph():
    """The 9-variable rank-deficient blankets of tests/test_big_blankets.py::test_dense_pipeline_truncating_eigen_route: a ring
    of 12 poses, three pendant poses measured in translation only; removing their anchors leaves targets that lose one
    direction beyond the gauge to the 1e-8 cut."""
    rng = np.random.default_rng(5)
    n = 15
    poses = np.zeros((n, 3))
    for i in range(12):
        a = 2 * np.pi * i / 12
        poses[i] = [5 * np.cos(a), 5 * np.sin(a), a + np.pi / 2]
    poses[12:] = poses[[2, 6, 9]] + rng.normal(scale=1.0, size=(3, 3))

    def rel(a, b):
        c, s = np.cos(poses[a, 2]), np.sin(poses[a, 2])
        dx, dy = poses[b, :2] - poses[a, :2]
        return np.array([c * dx + s * dy, -s * dx + c * dy, poses[b, 2] - poses[a, 2]]) + rng.normal(scale=0.01, size=3)
    full = np.diag([50.0, 50.0, 200.0])[np.triu_indices(3)]
    trans = np.diag([50.0, 50.0, 0.0])[np.triu_indices(3)]
    ij, data = [], []
    for i in range(12):
        ij.append((i, (i + 1) % 12)); data.append(np.concatenate([rel(i, (i + 1) % 12), full]))
    for p, a in zip((12, 13, 14), (2, 6, 9)):
        ij.append((a, p)); data.append(np.concatenate([rel(a, p), trans]))
    g = {"pose_dim": 3, "ids": np.arange(n, dtype=np.int32), "poses": poses, "edge_ij": np.array(ij, np.int32), "edge_data": np.array(data)}
    return g, np.array([2, 6, 9], np.int32)


def run_deficient(ctx):
    """-> (blankets, edges) without and with the flag"""
    from sparsifyposegraph_amd.graph import GraphWrapperHIP
    g, which = deficient_graph()
    out = []
    for flag in (False, True):
        hg = GraphWrapperHIP.from_dict(g, ctx=ctx, useGLC=True)
        st = hg.marginalizeNoOptimize(which, glc(3, abi.TOPO_DENSE, flag))
        assert st["n_bad_status"] == 0 and st["kld_sum"] == 0.0
        out.append((hg.blankets(), hg.edges()))
    return out


def check_skipped(out):
    (b0, e0), (b1, e1) = out
    for key in e0:
        assert np.array_equal(e0[key], e1[key]), key
    assert np.array_equal(b0["status"], b1["status"])
    assert np.isnan(b0["kld"]).all() and np.isnan(b1["kld"]).all()
    assert not (b0["info"] & abi.INFO_GLC_KLD_SKIPPED).any()
    assert (b1["info"] & abi.INFO_GLC_KLD_SKIPPED).all(), b1["info"]
    assert np.array_equal(b0["info"], b1["info"] & ~abi.INFO_GLC_KLD_SKIPPED)


@pytest.mark.gpu
def test_device_rank_deficient_blanket_is_skipped(hip_ctx):
    """The tail cut an eigenvalue (n - d - 1 rows): NaN + SPG_INFO_GLC_KLD_SKIPPED, edges as without the flag"""
    check_skipped(run_deficient(hip_ctx))


FORCED = '''
import os, sys
os.environ["SPG_FORCE_BIG"] = "1"
sys.path.insert(0, sys.argv[1])
from sparsifyposegraph_amd.lib import Context
from tests import test_glc_blanket_kld as t
ctx = Context(0)
ctx.profile(True)
out = t.run_deficient(ctx)
big = ctx.profile_read_big()
assert big["blankets"] == 6, big
t.check_skipped(out)
print("forced ok")
'''


@pytest.mark.gpu
def test_device_large_blanket_pipeline_is_skipped(tmp_path):
    """Every blanket forced through the dense HBM pipeline (SPG_FORCE_BIG=1, read once per process: own process), which does
    not compute the number: NaN + SPG_INFO_GLC_KLD_SKIPPED, edges as without the flag."""
    script = tmp_path / "forced_kld.py"
    script.write_text(FORCED)
    out = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "forced ok" in out.stdout
