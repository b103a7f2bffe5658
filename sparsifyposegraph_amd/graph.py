"""Host-side mirror of the reference's GraphWrapper / decimation interface over the C ABI.

Method names follow the reference (src/graph_wrapper.h:40-78, src/graph_wrapper_g2o.h:63-84,
src/decimation.h:18-22) so call sites read the same; the arithmetic lives in libspg_hip.so.
"""
import ctypes as C

import numpy as np

from . import abi, chi2
from .lib import Context, check, load

_f64p, _i32p, _i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)

# Context.set_linear_solver: SOLVER_PCG solves optimize()'s linear systems by preconditioned conjugate gradients
SOLVER_AUTO, SOLVER_DENSE, SOLVER_SPARSE, SOLVER_PCG = abi.SOLVER_AUTO, abi.SOLVER_DENSE, abi.SOLVER_SPARSE, abi.SOLVER_PCG


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class SparsityOptions:
    """src/sparsity_options.h:11-30 (defaults identical) plus the algorithm selector."""
    Tree, Subgraph, CliqueySubgraph, Dense, CliqueyDense = range(5)
    Local, Global = 0, 1

    def __init__(self, topology=0, chordRatio=1.0, linPoint=0, includeIntraClique=True):
        self.topology = topology
        self.chordRatio = chordRatio
        self.linPoint = linPoint
        self.includeIntraClique = includeIntraClique

    def to_abi(self, pose_dim, use_glc, flags=0):
        return abi.make_options(pose_dim, abi.ALG_GLC if use_glc else abi.ALG_NFR, self.topology,
                                self.linPoint, flags, self.chordRatio, int(self.includeIntraClique))


class DecimateOptions:
    def __init__(self, sparsity=2, clusterSize=1):
        self.sparsity = sparsity
        self.clusterSize = clusterSize


def _decimate(fn, last, endvert, opts):
    L = load()
    cap = max(endvert + 8, 16)
    out = np.zeros(cap, np.int32)
    n = getattr(L, fn)(int(last), int(endvert), int(opts.sparsity), int(opts.clusterSize), _p(out, C.c_int32), cap)
    return [int(x) for x in out[:n]]


def globalDecimate(last, endvert, opts):
    """src/decimation.cpp:36-49"""
    return _decimate("spg_decimate_global", last, endvert, opts)


def onlineDecimate(last, endvert, opts):
    """src/decimation.cpp:27-34"""
    return _decimate("spg_decimate_online", last, endvert, opts)


def clusterDecimate(last, endvert, opts):
    """src/decimation.cpp:11-25"""
    return _decimate("spg_decimate_cluster", last, endvert, opts)


class GraphWrapperHIP:
    """GraphWrapperG2O(verbose, useGLC) (src/graph_wrapper_g2o.cpp:102) with the marginalisation
    path, optimize() and the global KLD on the MI355X."""

    def __init__(self, ctx=None, pose_dim=6, useGLC=False, _handle=None):
        self.L = load()
        self.ctx = ctx if ctx is not None else Context()
        self.useGLC = bool(useGLC)
        if _handle is None:
            h = C.c_void_p()
            check(self.L.spg_graph_create(self.ctx.h, int(pose_dim), C.byref(h)), self.ctx.h, "spg_graph_create")
            _handle = h
        self.h = _handle
        self.d = self.L.spg_graph_pose_dim(self.h)
        self.last_stats = None
        self.glcBlanketKld = False   # setGlcBlanketKld
        self.factorDescent = False   # setFactorDescent
        self.ctx._track(self)

    # ---- construction -------------------------------------------------------------------
    @classmethod
    def load(cls, fname, ctx=None, useGLC=False):
        """GraphWrapperG2O(fname, optimize=false, useGLC) (src/graph_wrapper_g2o.cpp:107-154)"""
        ctx = ctx if ctx is not None else Context()
        h = C.c_void_p()
        check(load().spg_graph_load_g2o(ctx.h, fname.encode(), C.byref(h)), ctx.h, "spg_graph_load_g2o")
        return cls(ctx=ctx, useGLC=useGLC, _handle=h)

    @classmethod
    def from_dict(cls, g, ctx=None, useGLC=False):
        o = cls(ctx=ctx, pose_dim=g["pose_dim"], useGLC=useGLC)
        poses = np.ascontiguousarray(g["poses"], np.float64)
        ids = np.ascontiguousarray(g["ids"], np.int32)
        check(o.L.spg_graph_add_vertices(o.h, len(ids), _p(ids, C.c_int32), _p(poses, C.c_double)), o.ctx.h, "add_vertices")
        data = np.ascontiguousarray(g["edge_data"], np.float64)
        ij = np.ascontiguousarray(g["edge_ij"], np.int32)
        if len(ij):
            check(o.L.spg_graph_add_edges(o.h, len(ij), _p(ij, C.c_int32), _p(data, C.c_double)), o.ctx.h, "add_edges")
        return o

    def addVertex(self, id, init):
        init = np.ascontiguousarray(init, np.float64)
        check(self.L.spg_graph_add_vertex(self.h, int(id), _p(init, C.c_double)), self.ctx.h, "addVertex")

    def addEdge(self, frm, to, meas, info):
        """info: full d x d matrix or its row-wise upper triangle"""
        meas = np.ascontiguousarray(meas, np.float64)
        info = np.asarray(info, np.float64)
        if info.ndim == 2:
            info = info[np.triu_indices(self.d)]
        info = np.ascontiguousarray(info)
        check(self.L.spg_graph_add_edge(self.h, int(frm), int(to), _p(meas, C.c_double), _p(info, C.c_double)), self.ctx.h, "addEdge")

    def addGLCEdge(self, ids, meas, W):
        ids = np.ascontiguousarray(ids, np.int32)
        W = np.ascontiguousarray(W, np.float64)
        meas = np.ascontiguousarray(meas, np.float64)
        check(self.L.spg_graph_add_glc_edge(self.h, len(ids), _p(ids, C.c_int32), W.shape[0], _p(meas, C.c_double), _p(W, C.c_double)), self.ctx.h, "addGLCEdge")

    def addMultiEdge(self, ids, record):
        """MultiEdgeCorrelated over the vertices `ids` (src/multi_edge_correlated.hpp:28-63); `record` in the
        SPG_EDGE_MULTI layout of include/spg.h: nm | vertex pair of each measurement | measurements | W (information W^T W)."""
        ids = np.ascontiguousarray(ids, np.int32)
        record = np.ascontiguousarray(record, np.float64)
        check(self.L.spg_graph_add_multi_edge(self.h, len(ids), _p(ids, C.c_int32), _p(record, C.c_double), len(record)), self.ctx.h, "addMultiEdge")

    def setEstimate(self, vertexid, est):
        est = np.ascontiguousarray(est, np.float64)
        check(self.L.spg_graph_set_estimate(self.h, int(vertexid), _p(est, C.c_double)), self.ctx.h, "setEstimate")

    # ---- the hot path -------------------------------------------------------------------
    def setGlcBlanketKld(self, on=True):
        """Per-blanket KLD of GLC removals (SPG_FLAG_GLC_KLD, include/spg.h) in blankets()["kld"] and kld_sum for the
        marginalisations that follow; off by default, as in the reference. Only applies to SparsityOptions arguments of a
        useGLC graph: an abi.Options argument carries its own flags (abi.make_options(..., glc_kld=True))."""
        self.glcBlanketKld = bool(on)

    def setFactorDescent(self, on=True):
        """NFR blankets whose pattern has no closed form (Subgraph / Dense with more than k - 1 edges) by factor descent
        instead of the interior point (SPG_FLAG_NFR_FACTOR_DESCENT, include/spg.h; Context.set_factor_descent for the stop
        rule) in the marginalisations that follow; off by default. Only applies to SparsityOptions arguments of an NFR
        graph: an abi.Options argument carries its own flags (abi.make_options(..., factor_descent=True))."""
        self.factorDescent = bool(on)

    def _flags(self, flags):
        return flags | (abi.FLAG_GLC_KLD if (self.useGLC and self.glcBlanketKld) else 0) \
                     | (abi.FLAG_NFR_FACTOR_DESCENT if (not self.useGLC and self.factorDescent) else 0)

    def marginalizeNoOptimize(self, which, options, flags=0):
        """src/graph_wrapper_g2o.cpp:398-453"""
        which = np.ascontiguousarray(which, np.int32)
        o = options.to_abi(self.d, self.useGLC, self._flags(flags)) if isinstance(options, SparsityOptions) else options
        st = abi.MargStats()
        rc = self.L.spg_graph_marginalize(self.h, _p(which, C.c_int32), len(which), C.byref(o), C.byref(st))
        self.last_stats = st.asdict()
        check(rc, self.ctx.h, "spg_graph_marginalize")
        return self.last_stats

    def marginalize_ranks(self, which, options, rank, nranks, flags=0):
        """spg_graph_marginalize_ranks with the library's built-in exchange (the context's RCCL communicator,
        Context.ranks): every rank calls this with identical arguments on an identical replica."""
        which = np.ascontiguousarray(which, np.int32)
        o = options.to_abi(self.d, self.useGLC, self._flags(flags)) if isinstance(options, SparsityOptions) else options
        st = abi.MargStats()
        rc = self.L.spg_graph_marginalize_ranks(self.h, _p(which, C.c_int32), len(which), C.byref(o), int(rank), int(nranks), None, None, C.byref(st))
        self.last_stats = st.asdict()
        check(rc, self.ctx.h, "spg_graph_marginalize_ranks")
        return self.last_stats

    def marginalize(self, which, options, flags=0):
        """src/graph_wrapper_g2o.cpp:455-463: marginalizeNoOptimize followed by optimize() (dense LM up to 12 k
        variables, the block-sparse multifrontal solver beyond: `last_optimize_stats["solver"]`)."""
        st = self.marginalizeNoOptimize(which, options, flags)
        self.optimize()
        return st

    def computeSubstituteEdge(self, marginalized, maxid, frm, to):
        """src/compute_substitute_edge.cpp:13-96 -> (from, to, meas, info_upper)"""
        marg = np.ascontiguousarray(sorted(marginalized), np.int32)
        f, t = C.c_int(int(frm)), C.c_int(int(to))
        meas = np.zeros(abi.pose_stride(self.d))
        info = np.zeros(self.d * (self.d + 1) // 2)
        check(self.L.spg_graph_substitute_edge(self.h, _p(marg, C.c_int32), len(marg), int(maxid), C.byref(f), C.byref(t),
                                               _p(meas, C.c_double), _p(info, C.c_double)), self.ctx.h, "computeSubstituteEdge")
        return f.value, t.value, meas, info

    def optimize(self, iterations=50, fixed_id=-1):
        """GraphWrapperG2O::optimize (src/graph_wrapper_g2o.cpp:250-269): g2o Levenberg-Marquardt with
        the first vertex fixed, on the device (dense or block-sparse factorisation, see
        Context.set_linear_solver). Returns the stats dict."""
        st = abi.OptimizeStats()
        check(self.L.spg_graph_optimize(self.h, int(iterations), int(fixed_id), C.byref(st)), self.ctx.h, "optimize")
        self.last_optimize_stats = st.asdict()
        return self.last_optimize_stats

    def initialize(self, method=abi.INIT_CHORDAL, fixed_id=-1):
        """spg_graph_initialize: initial estimates from the measurements alone, the step before optimize() for a graph
        whose stored poses are poor. abi.INIT_CHORDAL: chordal relaxation on the device (rotations, projection, translations;
        two block-sparse factorisations); abi.INIT_SPANNING_TREE: g2o's computeInitialGuess on the host (any backend).
        The fixed vertex (fixed_id < 0: the smallest id) keeps its pose. Returns the stats dict."""
        st = abi.InitStats()
        check(self.L.spg_graph_initialize(self.h, int(method), int(fixed_id), C.byref(st)), self.ctx.h, "initialize")
        self.last_init_stats = st.asdict()
        return self.last_init_stats

    def chi2(self, other=None, iterations=50):
        """GraphWrapperG2O::chi2() / chi2(other) (src/graph_wrapper_g2o.cpp:501-529). Without `other`: the
        chi2 of the current estimates. With it: this graph's vertices that also exist in `other` are set
        to other's estimates and held fixed, the rest is optimised, chi2 is read and the estimates are
        restored (push / pop in the reference)."""
        if other is None:
            v = C.c_double()
            check(self.L.spg_graph_chi2(self.h, C.byref(v)), self.ctx.h, "chi2")
            return v.value
        ids, poses = self.vertices()
        mine = {int(i) for i in ids}
        oids, oposes = other.vertices()
        fixed = [int(i) for i in oids if int(i) in mine]
        for i, p in zip(oids, oposes):
            if int(i) in mine:
                self.setEstimate(int(i), p)
        fx = np.ascontiguousarray(sorted(set(fixed) | {int(ids[0])}), np.int32)
        st = abi.OptimizeStats()
        try:
            check(self.L.spg_graph_optimize_fixed(self.h, int(iterations), _p(fx, C.c_int32), len(fx), C.byref(st)), self.ctx.h, "chi2(other)")
        finally:
            for i, p in zip(ids, poses):
                self.setEstimate(int(i), p)
        return st.chi2_final

    def setRobustKernel(self, kind, delta=1.0, minIdGap=1):
        """g2o's setRobustKernel for the binary edges whose vertex ids are at least minIdGap apart (2 leaves
        consecutive-id odometry alone): abi.ROBUST_NONE / HUBER / CAUCHY / GEMAN_MCCLURE / DCS of width delta. optimize()
        and chi2(other) honour it (their chi2 is then sum rho); chi2(), information(), the covariances, the KLDs and the
        marginalisation never do. Clear it (ROBUST_NONE) before optimising a sparsified graph."""
        check(self.L.spg_graph_set_robust_kernel(self.h, int(kind), float(delta), int(minIdGap)), self.ctx.h, "setRobustKernel")

    def robustKernel(self):
        """(kind, delta, minIdGap) as set by setRobustKernel"""
        k, g, d = C.c_int(), C.c_int(), C.c_double()
        check(self.L.spg_graph_get_robust_kernel(self.h, C.byref(k), C.byref(d), C.byref(g)), self.ctx.h, "robustKernel")
        return k.value, d.value, g.value

    def edgeChi2(self):
        """Per edge, in the order of edges(), at the stored estimates: (chi2, rho, weight) — the plain e^T Omega e (n-ary
        edges: ||W e||^2), and rho / weight of the graph's robust kernel (chi2 and 1 without one and for exempt edges)."""
        n = self.L.spg_graph_edge_chi2(self.h, None, None, None, 0)
        check(n, self.ctx.h, "edgeChi2")
        s, rho, w = np.zeros(max(n, 1)), np.zeros(max(n, 1)), np.zeros(max(n, 1))
        check(self.L.spg_graph_edge_chi2(self.h, _p(s, C.c_double), _p(rho, C.c_double), _p(w, C.c_double), n), self.ctx.h, "edgeChi2")
        return s[:n], rho[:n], w[:n]

    def information(self, fixed_id=-1):
        """GraphWrapperG2O::information (src/graph_wrapper_g2o.cpp:351-358): dense Gauss-Newton
        information at the stored estimates, all vertices but the fixed one (default: smallest id)."""
        n = self.L.spg_graph_information(self.h, int(fixed_id), None, 0)
        check(min(int(n), 0), self.ctx.h, "information")
        out = np.zeros((int(n), int(n)))
        rc = self.L.spg_graph_information(self.h, int(fixed_id), _p(out, C.c_double), out.size)
        check(min(int(rc), 0), self.ctx.h, "information")
        return out

    def sparseInformation(self, fixed_id=-1, values=True):
        """GraphWrapperG2O::sparseInformation (src/graph_wrapper_g2o.cpp:382-396): information() in block-CSR form at any
        size. Returns (indptr int64[nb + 1], indices int32[nnzb], blocks float64[nnzb, D, D], ids int32[nb]) — the first
        three are the arguments of scipy.sparse.bsr_matrix((blocks, indices, indptr)); ids names the block rows. Both
        triangles are stored, block (u, v) is the transpose of block (v, u) bit for bit. values=False: the pattern only
        (host work, blocks is None)."""
        d = self.d
        nnzb = self.L.spg_graph_sparse_information(self.h, int(fixed_id), None, None, None, 0, None)
        check(min(int(nnzb), 0), self.ctx.h, "sparseInformation")
        nb = self.numVertices() - 1
        indptr, indices = np.zeros(nb + 1, np.int64), np.zeros(max(int(nnzb), 1), np.int32)
        blocks = np.zeros((max(int(nnzb), 1), d, d)) if values else None
        ids = np.zeros(max(nb, 1), np.int32)
        rc = self.L.spg_graph_sparse_information(self.h, int(fixed_id), _p(indptr, C.c_int64), _p(indices, C.c_int32),
                                                 _p(blocks, C.c_double) if values else None, int(nnzb), _p(ids, C.c_int32))
        check(min(int(rc), 0), self.ctx.h, "sparseInformation")
        return indptr, indices[:int(nnzb)], (blocks[:int(nnzb)] if values else None), ids[:nb]

    def informationApply(self, X, fixed_id=-1):
        """H @ X with H = information(fixed_id), assembled block-CSR on the device and never formed densely. X: float64[n]
        or float64[nrhs, n] (one vector per row), n = D * (vertices - 1); returns the same shape."""
        X = np.ascontiguousarray(X, np.float64)
        n = self.d * (self.numVertices() - 1)
        if X.ndim not in (1, 2) or X.shape[-1] != n:
            raise ValueError(f"informationApply: X must be [{n}] or [nrhs, {n}], got {X.shape}")
        Y = np.zeros_like(X)
        nrhs = 1 if X.ndim == 1 else X.shape[0]
        if n > 0 or nrhs <= 0:
            check(self.L.spg_graph_information_apply(self.h, int(fixed_id), _p(X, C.c_double), nrhs, _p(Y, C.c_double)), self.ctx.h, "informationApply")
        return Y

    def covariance(self, fixed_id=-1):
        """GraphWrapperG2O::covariance (src/graph_wrapper_g2o.cpp:368-373): inverse of information(), dense on
        the device (blocked fp64-MFMA Cholesky, triangular inverse, L^-T L^-1)."""
        n = self.L.spg_graph_covariance(self.h, int(fixed_id), None, 0)
        check(min(int(n), 0), self.ctx.h, "covariance")
        out = np.zeros((int(n), int(n)))
        rc = self.L.spg_graph_covariance(self.h, int(fixed_id), _p(out, C.c_double), out.size)
        check(min(int(rc), 0), self.ctx.h, "covariance")
        return out

    def clonePortion(self, maxid, optimize=True):
        """GraphWrapperG2O::clonePortion (src/graph_wrapper_g2o.cpp:334-356): vertices / edges up to maxid on the
        same context; the reference optimises the clone before returning it."""
        h = C.c_void_p()
        check(self.L.spg_graph_clone_portion(self.h, int(maxid), C.byref(h)), self.ctx.h, "clonePortion")
        gw = GraphWrapperHIP(ctx=self.ctx, useGLC=self.useGLC, _handle=h)
        if optimize and gw.numVertices() > 1 and gw.numEdges() > 0:
            gw.optimize()
        return gw

    def vertexEdges(self, vertexid):
        """GraphWrapper::Vertex::edges() (src/graph_wrapper.h:26): indices into edges() of the edges at the vertex"""
        n = self.L.spg_graph_vertex_edges(self.h, int(vertexid), None, 0)
        check(n, self.ctx.h, "vertexEdges")
        out = np.zeros(max(n, 1), np.int32)
        check(self.L.spg_graph_vertex_edges(self.h, int(vertexid), _p(out, C.c_int32), n), self.ctx.h, "vertexEdges")
        return out[:n]

    def writeString(self):
        """GraphWrapper::write(std::ofstream &) (src/graph_wrapper.h:62): the .g2o text"""
        txt, ln = C.c_void_p(), C.c_size_t()
        check(self.L.spg_graph_write_g2o_mem(self.h, C.byref(txt), C.byref(ln)), self.ctx.h, "write")
        try:
            return C.string_at(txt.value, ln.value).decode()
        finally:
            self.L.spg_free(txt)

    def kullbackLeibler(self, other, fixed_id=-1):
        """GraphWrapperG2O::kullbackLeibler(other) called on the baseline
        (src/graph_wrapper_g2o.cpp:531-548). Returns the KLD; the terms are in `last_kld_terms`."""
        t = abi.KldTerms()
        check(self.L.spg_graph_kullback_leibler(self.h, other.h, int(fixed_id), C.byref(t)), self.ctx.h, "kullbackLeibler")
        self.last_kld_terms = t.asdict()
        return t.kld

    def marginalCovariances(self, ids=None, fixed_id=-1):
        """GraphWrapperISAM::covariance (src/graph_wrapper_isam.cpp:259-262): the marginal covariance of each vertex,
        read from the selected inverse of the sparse factor. ids=None: every vertex, ascending id. Returns
        (ids, float64[n, D, D]); the fixed vertex's block is zero. Stats in `last_covariance_stats`."""
        d, st = self.d, abi.CovStats()
        if ids is None:
            ids = self.vertices()[0]
            ip = None
        else:
            ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
            ip = _p(ids, C.c_int32)
        n = self.L.spg_graph_marginal_covariances(self.h, int(fixed_id), ip, len(ids), None, 0, None)
        check(min(int(n), 0), self.ctx.h, "marginalCovariances")
        out = np.zeros((int(n) // (d * d), d, d))
        rc = self.L.spg_graph_marginal_covariances(self.h, int(fixed_id), ip, len(ids), _p(out, C.c_double), out.size, C.byref(st))
        check(min(int(rc), 0), self.ctx.h, "marginalCovariances")
        self.last_covariance_stats = st.asdict()
        return np.asarray(ids, np.int32), out

    def jointCovariances(self, pairs, fixed_id=-1):
        """The 2D x 2D covariance [[Saa, Sab], [Sba, Sbb]] of each pair (a, b) of vertices that share a live edge, from
        the selected inverse of the sparse factor. Returns float64[n, 2D, 2D]. Stats in `last_covariance_stats`."""
        d, st = self.d, abi.CovStats()
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = self.L.spg_graph_joint_covariances(self.h, int(fixed_id), _p(pr, C.c_int32), len(pr), None, 0, None)
        check(min(int(n), 0), self.ctx.h, "jointCovariances")
        out = np.zeros((len(pr), 2 * d, 2 * d))
        rc = self.L.spg_graph_joint_covariances(self.h, int(fixed_id), _p(pr, C.c_int32), len(pr), _p(out, C.c_double), out.size, C.byref(st))
        check(min(int(rc), 0), self.ctx.h, "jointCovariances")
        self.last_covariance_stats = st.asdict()
        return out

    def pairCovariances(self, pairs, fixed_id=-1):
        """The 2D x 2D covariance [[Saa, Sab], [Sba, Sbb]] of each pair (a, b) of distinct vertices, with or without a
        common edge: in-pattern blocks from the selected inverse, the others from column solves through the sparse
        factor. Returns float64[n, 2D, 2D]. Stats (abi.CovSolveStats) in `last_covariance_stats`."""
        d, st = self.d, abi.CovSolveStats()
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = self.L.spg_graph_pair_covariances(self.h, int(fixed_id), _p(pr, C.c_int32), len(pr), None, 0, None)
        check(min(int(n), 0), self.ctx.h, "pairCovariances")
        out = np.zeros((len(pr), 2 * d, 2 * d))
        rc = self.L.spg_graph_pair_covariances(self.h, int(fixed_id), _p(pr, C.c_int32), len(pr), _p(out, C.c_double), out.size, C.byref(st))
        check(min(int(rc), 0), self.ctx.h, "pairCovariances")
        self.last_covariance_stats = st.asdict()
        return out

    def jointMarginalCovariance(self, ids, fixed_id=-1):
        """GraphWrapperISAM::covariance (src/graph_wrapper_isam.cpp:259-262), covariances().marginal(ids): the (nD) x (nD)
        joint covariance of n distinct vertices in the order given; off-diagonal blocks mirrored exactly. Returns float64[nD, nD]. Stats
        (abi.CovSolveStats) in `last_covariance_stats`."""
        d, st = self.d, abi.CovSolveStats()
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        n = self.L.spg_graph_joint_marginal_covariance(self.h, int(fixed_id), _p(ids, C.c_int32), len(ids), None, 0, None)
        check(min(int(n), 0), self.ctx.h, "jointMarginalCovariance")
        out = np.zeros((len(ids) * d, len(ids) * d))
        rc = self.L.spg_graph_joint_marginal_covariance(self.h, int(fixed_id), _p(ids, C.c_int32), len(ids), _p(out, C.c_double), out.size,
                                                        C.byref(st))
        check(min(int(rc), 0), self.ctx.h, "jointMarginalCovariance")
        self.last_covariance_stats = st.asdict()
        return out

    def relativeCovariances(self, pairs, fixed_id=-1):
        """The covariance of the relative pose Xa^-1 Xb of each pair (a, b) of distinct vertices: P = J Sigma_ab J^T with J
        the Jacobians of the binary edge a -> b measured at the current relative pose (include/spg.h). The pair blocks stay
        on the device. Returns (rel float64[n, 3|7], cov float64[n, D, D]); rel[i] and inv(cov[i]) are a record addEdge
        accepts. Stats (abi.CovSolveStats) in `last_covariance_stats`."""
        d, st = self.d, abi.CovSolveStats()
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = self.L.spg_graph_relative_covariances(self.h, int(fixed_id), _p(pr, C.c_int32), len(pr), None, None, 0, None)
        check(min(int(n), 0), self.ctx.h, "relativeCovariances")
        rel, cov = np.zeros((len(pr), 3 if d == 3 else 7)), np.zeros((len(pr), d, d))
        rc = self.L.spg_graph_relative_covariances(self.h, int(fixed_id), _p(pr, C.c_int32), len(pr), _p(rel, C.c_double), _p(cov, C.c_double),
                                                   cov.size, C.byref(st))
        check(min(int(rc), 0), self.ctx.h, "relativeCovariances")
        self.last_covariance_stats = st.asdict()
        return rel, cov

    def scoreCandidates(self, ij, meas, info_upper, fixed_id=-1):
        """Scores n hypothetical binary edges ij[k, 0] -> ij[k, 1] with measurement meas[k] (3|7) and information
        info_upper[k] (upper triangle, the layout of addEdge) against the graph, without modifying it (include/spg.h):
        d2 = the innovation Mahalanobis distance e^T (P + Omega^-1)^-1 e (chi^2 with D degrees of freedom for an inlier),
        gain = the information gain 1/2 ln det(I + Omega P) in nats, chi2 = e^T Omega e, status = abi.CAND_SCORED or
        abi.CAND_INFO_NOT_PD (the three values are NaN). Returns a dict of arrays. Stats in `last_covariance_stats`."""
        d, st = self.d, abi.CovSolveStats()
        ij = np.ascontiguousarray(ij, np.int32).reshape(-1, 2)
        n = len(ij)
        rec = np.ascontiguousarray(np.concatenate([np.asarray(meas, np.float64).reshape(n, -1), np.asarray(info_upper, np.float64).reshape(n, -1)],
                                                  axis=1))
        if rec.shape[1] != (3 if d == 3 else 7) + d * (d + 1) // 2:
            raise ValueError("scoreCandidates: meas must be n x (3|7) and info_upper n x D (D + 1) / 2")
        out = {"d2": np.zeros(n), "gain": np.zeros(n), "chi2": np.zeros(n), "status": np.zeros(n, np.int32)}
        rc = self.L.spg_graph_score_candidates(self.h, int(fixed_id), _p(ij, C.c_int32), _p(rec, C.c_double), n, _p(out["d2"], C.c_double),
                                               _p(out["gain"], C.c_double), _p(out["chi2"], C.c_double), _p(out["status"], C.c_int32), n,
                                               C.byref(st))
        check(min(int(rc), 0), self.ctx.h, "scoreCandidates")
        self.last_covariance_stats = st.asdict()
        return out

    def selectCandidates(self, ij, meas, info_upper, k, min_gain=0.0, max_d2=0.0, fixed_id=-1):
        """Greedy choice of up to k of the n candidates of scoreCandidates' layout by conditional information gain
        (include/spg.h: spg_graph_select_candidates): each round takes the candidate with the largest gain given the ones
        already chosen (ties: the lowest index), on the device, without modifying the graph. max_d2 > 0 gates on the d2 of
        the graph as it stands (evaluated once); selection stops early when the best gain is < min_gain or nothing is
        eligible. Returns a dict: selected int32[r] (indices into the list, in order), cond_gain float64[r], final_gain
        float64[n] (NaN for selected, gated and not-PD candidates), status int32[n] (abi.CAND_*). Stats
        (abi.SelectStats) in `last_covariance_stats`."""
        d, st = self.d, abi.SelectStats()
        ij = np.ascontiguousarray(ij, np.int32).reshape(-1, 2)
        n = len(ij)
        ps, tri = (3 if d == 3 else 7), d * (d + 1) // 2
        meas, info_upper = np.asarray(meas, np.float64), np.asarray(info_upper, np.float64)
        if meas.size != n * ps or info_upper.size != n * tri:
            raise ValueError("selectCandidates: meas must be n x (3|7) and info_upper n x D (D + 1) / 2")
        rec = np.ascontiguousarray(np.concatenate([meas.reshape(n, ps), info_upper.reshape(n, tri)], axis=1))
        cap = max(min(int(k), n), 0)
        sel, cg = np.full(max(cap, 1), -1, np.int32), np.full(max(cap, 1), np.nan)
        out = {"final_gain": np.full(n, np.nan), "status": np.zeros(n, np.int32)}
        rc = self.L.spg_graph_select_candidates(self.h, int(fixed_id), _p(ij, C.c_int32), _p(rec, C.c_double), n, int(k), float(min_gain),
                                                float(max_d2), _p(sel, C.c_int32), _p(cg, C.c_double), cap, _p(out["final_gain"], C.c_double),
                                                _p(out["status"], C.c_int32), C.byref(st))
        check(min(int(rc), 0), self.ctx.h, "selectCandidates")
        self.last_covariance_stats = st.asdict()
        out["selected"], out["cond_gain"] = sel[:rc].copy(), cg[:rc].copy()
        return out

    def compatibleCandidates(self, ij, meas, info_upper, k=None, significance=0.99, max_d2=None, pair_max_d2=None, joint_max_d2=None, pairs=False,
                             fixed_id=-1):
        """Which of the n candidates of scoreCandidates' layout agree with each other (include/spg.h:
        spg_graph_compatible_candidates), on the device, without modifying the graph: the joint Mahalanobis distance of
        every pair of gated candidates against pair_max_d2 gives a consistency graph, a greedy search over every seed its
        largest consistent set, and the members of that set pass a sequential joint gate in ascending d2 (member p + 1
        against joint_max_d2[p]) until k are accepted (k=None: n). Thresholds left None come from `significance`: the
        chi^2 quantile with D degrees of freedom for max_d2 (0 = no gate), 2D for pair_max_d2, pD, p = 1 .. min(k, n),
        for joint_max_d2 (False = no joint gate). Returns a dict: compatible int32[r] (indices into the list, in order of
        acceptance), joint_d2 float64[r] (the joint distance after each), clique int32[c] (the consistent set in order of
        construction), d2 float64[n], degree int32[n], status int32[n] (abi.CAND_*), pair_d2 float64[n, n] when `pairs`,
        and the thresholds used. Stats (abi.CompatStats) in `last_covariance_stats`."""
        d, st = self.d, abi.CompatStats()
        ij = np.ascontiguousarray(ij, np.int32).reshape(-1, 2)
        n = len(ij)
        ps, tri = (3 if d == 3 else 7), d * (d + 1) // 2
        meas, info_upper = np.asarray(meas, np.float64), np.asarray(info_upper, np.float64)
        if meas.size != n * ps or info_upper.size != n * tri:
            raise ValueError("compatibleCandidates: meas must be n x (3|7) and info_upper n x D (D + 1) / 2")
        rec = np.ascontiguousarray(np.concatenate([meas.reshape(n, ps), info_upper.reshape(n, tri)], axis=1))
        k = n if k is None else int(k)
        cap = max(min(k, n), 0)
        q = float(significance)
        if max_d2 is None:
            max_d2 = chi2.chi2_quantile(q, d)
        if pair_max_d2 is None:
            pair_max_d2 = chi2.chi2_quantile(q, 2 * d)
        if joint_max_d2 is None:
            joint_max_d2 = chi2.chi2_quantile_table(q, d, cap)
        jm = None
        if joint_max_d2 is not False:
            jm = np.ascontiguousarray(joint_max_d2, np.float64).reshape(-1)
            if len(jm) < cap:
                raise ValueError("compatibleCandidates: joint_max_d2 must have min(k, n) entries")
        sel, jd = np.full(max(cap, 1), -1, np.int32), np.full(max(cap, 1), np.nan)
        clique = np.full(max(n, 1), -1, np.int32)
        out = {"d2": np.full(n, np.nan), "degree": np.zeros(n, np.int32), "status": np.zeros(n, np.int32)}
        pd = np.full((n, n), np.nan) if pairs else None
        rc = self.L.spg_graph_compatible_candidates(self.h, int(fixed_id), _p(ij, C.c_int32), _p(rec, C.c_double), n, k, float(max_d2),
                                                    float(pair_max_d2), None if jm is None else _p(jm, C.c_double), _p(sel, C.c_int32),
                                                    _p(jd, C.c_double), cap, _p(clique, C.c_int32), n, _p(out["d2"], C.c_double),
                                                    _p(out["degree"], C.c_int32), _p(out["status"], C.c_int32),
                                                    None if pd is None else _p(pd, C.c_double), n * n, C.byref(st))
        check(min(int(rc), 0), self.ctx.h, "compatibleCandidates")
        self.last_covariance_stats = st.asdict()
        out["compatible"], out["joint_d2"] = sel[:rc].copy(), jd[:rc].copy()
        out["clique"] = clique[:max(st.clique_size, 0)].copy()
        out["max_d2"], out["pair_max_d2"], out["joint_max_d2"] = float(max_d2), float(pair_max_d2), None if jm is None else jm[:cap].copy()
        if pairs:
            out["pair_d2"] = pd
        return out

    def proposeCandidates(self, search_radius, max_angle=0.0, min_id_gap=1, max_per_vertex=0, queries=None, range=0.0, z_max=2.0, fixed_id=-1,
                          stats=False):
        """Loop-closure candidates by proximity and range (include/spg.h: spg_graph_propose_candidates), on the device,
        without modifying the graph. Stage A: the pairs of distinct live vertices within search_radius of each other (and
        within max_angle when > 0, at least min_id_gap ids apart when > 1, without a common live edge, with an endpoint in
        `queries` when given), at most the max_per_vertex nearest per query vertex (0: all; symmetrised), found on a
        uniform grid. Stage B, when range > 0: a pair stays iff zscore = (rho - range) / sigma <= z_max, sigma the
        standard deviation of the pair's range from its relative covariance in the gauge of fixed_id; the cap of stage A
        applies first. Returns a dict of numpy arrays in ascending (id_a, id_b) order: ij int32[n, 2], dist, angle
        float64[n], with range > 0 also sigma and zscore; with `stats` the entry "stats" (abi.ProposeStats.asdict())."""
        st = abi.ProposeStats()
        q, nq = None, 0
        if queries is not None:
            q = np.ascontiguousarray(queries, np.int32).reshape(-1)
            nq = len(q)
        gate = float(range) > 0.0

        def call(rng, cap, ij, dist, angle, sigma, zscore, q=q, nq=nq):
            rc = self.L.spg_graph_propose_candidates(self.h, int(fixed_id), float(search_radius), float(max_angle), int(min_id_gap), int(max_per_vertex),
                                                     None if q is None else _p(q, C.c_int32), nq, rng, float(z_max),
                                                     None if ij is None else _p(ij, C.c_int32), None if dist is None else _p(dist, C.c_double),
                                                     None if angle is None else _p(angle, C.c_double), None if sigma is None else _p(sigma, C.c_double),
                                                     None if zscore is None else _p(zscore, C.c_double), cap, C.byref(st))
            check(min(int(rc), 0), self.ctx.h, "proposeCandidates")
            return int(rc)
        # the size query runs stage A alone (no fill, no covariance): the gate can only drop pairs of it. Before it, with an
        # empty query list, the call checks range with the other arguments and returns 0 without touching the backend.
        if gate:
            call(float(range), 0, None, None, None, None, None, q=np.zeros(1, np.int32), nq=0)
        cap = call(0.0 if gate else float(range), 0, None, None, None, None, None)
        ij, dist, angle = np.zeros((max(cap, 1), 2), np.int32), np.zeros(max(cap, 1)), np.zeros(max(cap, 1))
        sigma, zscore = (np.zeros(max(cap, 1)), np.zeros(max(cap, 1))) if gate else (None, None)
        n = call(float(range), cap, ij, dist, angle, sigma, zscore) if cap > 0 else 0
        out = {"ij": ij[:n].copy(), "dist": dist[:n].copy(), "angle": angle[:n].copy()}
        if gate:
            out["sigma"], out["zscore"] = sigma[:n].copy(), zscore[:n].copy()
        self.last_covariance_stats = st.asdict()
        if stats:
            out["stats"] = st.asdict()
        return out

    def selectRemovals(self, radius, max_angle=0.0, keep=(), priority=None, stats=False):
        """The vertices to remove by spatial redundancy (include/spg.h: spg_graph_select_removals), on the device, without
        modifying the graph: one pose is kept per neighbourhood of `radius` (and of `max_angle` when > 0). `keep`: ids
        that stay whatever happens. `priority` decides who stays among the others, the higher value first, ties to the
        lower id: None (a hash of the id: no order along the trajectory, the fewest rounds), "oldest" (-id), "newest" (+id),
        an array with one value per live vertex in ascending-id order, or a dict id -> value over the live ids. Returns
        (removed, representative, rep_dist): int32[r] ascending ids, ready for marginalize(), for each the kept vertex nearest
        to it, and the distance; with `stats` also abi.RemovalStats.asdict()."""
        st = abi.RemovalStats()
        kp = np.ascontiguousarray(keep, np.int32).reshape(-1)
        pr = None
        if priority is not None:
            ids = np.sort(self.vertices()[0])
            if isinstance(priority, str):
                if priority not in ("oldest", "newest"):
                    raise ValueError('selectRemovals: priority is None, "oldest", "newest", an array or a dict')
                pr = ids.astype(np.float64) * (-1.0 if priority == "oldest" else 1.0)
            elif isinstance(priority, dict):
                missing = [int(i) for i in ids if int(i) not in priority]
                if missing:
                    raise ValueError(f"selectRemovals: priority has no value for vertex {missing[0]}")
                pr = np.array([priority[int(i)] for i in ids], np.float64)
            else:
                pr = np.ascontiguousarray(priority, np.float64).reshape(-1)
                if len(pr) != len(ids):
                    raise ValueError(f"selectRemovals: priority has {len(pr)} entries for {len(ids)} live vertices")

        def call(cap, rem, rep, rd):
            rc = self.L.spg_graph_select_removals(self.h, float(radius), float(max_angle), _p(kp, C.c_int32) if len(kp) else None, len(kp),
                                                  None if pr is None else _p(pr, C.c_double), None if rem is None else _p(rem, C.c_int32),
                                                  None if rep is None else _p(rep, C.c_int32), None if rd is None else _p(rd, C.c_double), cap,
                                                  C.byref(st))
            check(min(int(rc), 0), self.ctx.h, "selectRemovals")
            return int(rc)
        # one call: the decision is the whole cost, and no more than every live vertex can be removed
        cap = max(self.numVertices(), 1)
        rem, rep, rd = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap)
        n = call(cap, rem, rep, rd)
        out = (rem[:n].copy(), rep[:n].copy(), rd[:n].copy())
        return out + (st.asdict(),) if stats else out

    def pruneCandidates(self, edge_idx, k, max_loss=0.0, max_kld=0.0, min_margin=0.0, fixed_id=-1):
        """Greedy choice of up to k of the listed live binary edges (indices into the order of edges()) by conditional
        information loss (include/spg.h: spg_graph_prune_candidates): each round takes the edge whose removal costs the
        least given the ones already taken (ties: the lowest index), on the device, without modifying the graph. An edge
        whose removal would make the information singular to min_margin (<= 0: 1e-6) is not eligible; that is re-evaluated
        every round. Stops early on max_loss / max_kld (<= 0: no limit). Returns a dict: pruned int32[r] (indices into
        edge_idx, in order), cond_loss float64[r], kld float64[r] (cumulative, exact at the stored estimates), final_loss,
        final_margin float64[n], status int32[n] (abi.PRUNE_*). Stats (abi.PruneStats) in `last_covariance_stats`."""
        st = abi.PruneStats()
        idx = np.ascontiguousarray(edge_idx, np.int32).reshape(-1)
        n = len(idx)
        cap = max(min(int(k), n), 0)
        sel, cl, ck = np.full(max(cap, 1), -1, np.int32), np.full(max(cap, 1), np.nan), np.full(max(cap, 1), np.nan)
        out = {"final_loss": np.full(n, np.nan), "final_margin": np.full(n, np.nan), "status": np.zeros(n, np.int32)}
        rc = self.L.spg_graph_prune_candidates(self.h, int(fixed_id), _p(idx, C.c_int32), n, int(k), float(max_loss), float(max_kld),
                                               float(min_margin), _p(sel, C.c_int32), _p(cl, C.c_double), _p(ck, C.c_double), cap,
                                               _p(out["final_loss"], C.c_double), _p(out["final_margin"], C.c_double),
                                               _p(out["status"], C.c_int32), C.byref(st))
        check(min(int(rc), 0), self.ctx.h, "pruneCandidates")
        self.last_covariance_stats = st.asdict()
        out["pruned"], out["cond_loss"], out["kld"] = sel[:rc].copy(), cl[:rc].copy(), ck[:rc].copy()
        return out

    def removeEdges(self, edge_idx):
        """Removes the listed live edges (indices into the order of edges(), any kind); the others keep their order
        (include/spg.h: spg_graph_remove_edges)."""
        idx = np.ascontiguousarray(edge_idx, np.int32).reshape(-1)
        check(self.L.spg_graph_remove_edges(self.h, _p(idx, C.c_int32), len(idx)), self.ctx.h, "removeEdges")

    def pruneEdges(self, edge_idx, k, max_loss=0.0, max_kld=0.0, min_margin=0.0, fixed_id=-1):
        """pruneCandidates followed by removeEdges of what it chose; returns pruneCandidates' dict."""
        idx = np.ascontiguousarray(edge_idx, np.int32).reshape(-1)
        out = self.pruneCandidates(idx, k, max_loss, max_kld, min_margin, fixed_id)
        self.removeEdges(idx[out["pruned"]])
        return out

    def detectOutliers(self, edge_idx, k, min_stat=0.0, significance=None, min_margin=0.0, fixed_id=-1):
        """Greedy data snooping over the listed live binary edges (indices into the order of edges(); include/spg.h:
        spg_graph_detect_outliers): each round flags the edge with the largest leave-one-out chi^2 statistic given the ones
        already flagged (ties: the lowest index) and re-conditions the others, on the device, without modifying the graph.
        The stored estimates are taken as the minimiser: call optimize() first. Stops when the best statistic is < min_stat
        (<= 0: no threshold); significance=p sets min_stat to the chi^2_D quantile at 1 - p. An edge whose removal would
        make the information singular to min_margin (<= 0: 1e-6) cannot be tested. Returns a dict: flagged int32[r]
        (indices into edge_idx, in order), stat float64[r], final_stat, final_margin, redundancy float64[n], status
        int32[n] (abi.OUTLIER_*). Stats (abi.OutlierStats) in `last_covariance_stats`."""
        if significance is not None:
            min_stat = chi2.chi2_quantile(1.0 - float(significance), self.d)
        st = abi.OutlierStats()
        idx = np.ascontiguousarray(edge_idx, np.int32).reshape(-1)
        n = len(idx)
        cap = max(min(int(k), n), 0)
        sel, cs = np.full(max(cap, 1), -1, np.int32), np.full(max(cap, 1), np.nan)
        out = {"final_stat": np.full(n, np.nan), "final_margin": np.full(n, np.nan), "redundancy": np.full(n, np.nan),
               "status": np.zeros(n, np.int32)}
        rc = self.L.spg_graph_detect_outliers(self.h, int(fixed_id), _p(idx, C.c_int32), n, int(k), float(min_stat), float(min_margin),
                                              _p(sel, C.c_int32), _p(cs, C.c_double), cap, _p(out["final_stat"], C.c_double),
                                              _p(out["final_margin"], C.c_double), _p(out["redundancy"], C.c_double),
                                              _p(out["status"], C.c_int32), C.byref(st))
        check(min(int(rc), 0), self.ctx.h, "detectOutliers")
        self.last_covariance_stats = st.asdict()
        out["flagged"], out["stat"], out["min_stat"] = sel[:rc].copy(), cs[:rc].copy(), float(min_stat)
        return out

    def rejectOutliers(self, edge_idx, k, min_stat=0.0, significance=None, min_margin=0.0, fixed_id=-1):
        """detectOutliers followed by removeEdges of what it flagged; returns detectOutliers' dict."""
        idx = np.ascontiguousarray(edge_idx, np.int32).reshape(-1)
        out = self.detectOutliers(idx, k, min_stat, significance, min_margin, fixed_id)
        self.removeEdges(idx[out["flagged"]])
        return out

    def marginalKullbackLeibler(self, other, fixed_id=-1):
        """Called on the baseline: kullbackLeiblerDivergence (src/utils.cpp:70-97) of each vertex's marginal in `other`
        against its marginal here, for every vertex of `other` but the fixed one. Returns (ids, kld), ascending ids.
        Stats in `last_covariance_stats`."""
        st = abi.CovStats()
        n = self.L.spg_graph_marginal_kld(self.h, other.h, int(fixed_id), None, None, 0, None)
        check(n, self.ctx.h, "marginalKullbackLeibler")
        ids, kld = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1))
        rc = self.L.spg_graph_marginal_kld(self.h, other.h, int(fixed_id), _p(ids, C.c_int32), _p(kld, C.c_double), n, C.byref(st))
        check(rc, self.ctx.h, "marginalKullbackLeibler")
        self.last_covariance_stats = st.asdict()
        return ids[:n], kld[:n]

    # round-stepping form (multi-GPU driver in parallel.py)
    def begin(self, which, opts, rank, nranks):
        which = np.ascontiguousarray(which, np.int32)
        self._opts = opts
        check(self.L.spg_graph_marginalize_begin(self.h, _p(which, C.c_int32), len(which), C.byref(opts), rank, nranks), self.ctx.h, "marginalize_begin")

    def set_shard_threshold(self, min_blankets):
        check(self.L.spg_graph_set_shard_threshold(self.h, int(min_blankets)), self.ctx.h, "set_shard_threshold")

    def set_stream_emulation(self, seed):
        """-1: default drivers; >= 0: streaming driver on an injected backend, completion order from the seed (tests);
        -2: never use the streaming driver (A/B against the batch driver)."""
        check(self.L.spg_graph_set_stream_emulation(self.h, int(seed)), self.ctx.h, "set_stream_emulation")

    def round_prepare(self):
        info = abi.RoundInfo()
        rc = check(self.L.spg_graph_round_prepare(self.h, C.byref(info)), self.ctx.h, "round_prepare")
        return info if rc == 1 else None

    def round_compute(self):
        check(self.L.spg_graph_round_compute(self.h), self.ctx.h, "round_compute")

    def round_commit(self):
        check(self.L.spg_graph_round_commit(self.h), self.ctx.h, "round_commit")

    def end(self):
        st = abi.MargStats()
        rc = self.L.spg_graph_marginalize_end(self.h, C.byref(st))
        self.last_stats = st.asdict()
        check(rc, self.ctx.h, "marginalize_end")
        return self.last_stats

    def arena(self):
        cap = C.c_int64()
        p = self.L.spg_graph_arena(self.h, C.byref(cap))
        return p, cap.value

    def reserve(self, doubles):
        check(self.L.spg_graph_reserve(self.h, int(doubles)), self.ctx.h, "reserve")

    # ---- queries ------------------------------------------------------------------------
    def numVertices(self):
        return self.L.spg_graph_num_vertices(self.h)

    def numEdges(self):
        return self.L.spg_graph_num_edges(self.h)

    def vertices(self):
        n = self.numVertices()
        ids = np.zeros(n, np.int32)
        poses = np.zeros((n, abi.pose_stride(self.d)))
        check(self.L.spg_graph_get_vertices(self.h, _p(ids, C.c_int32), _p(poses, C.c_double)), self.ctx.h, "get_vertices")
        return ids, poses

    def edges(self):
        ne = self.numEdges()
        nd = self.L.spg_graph_edge_data_size(self.h)
        nv = self.L.spg_graph_edge_vert_size(self.h)
        kind = np.zeros(ne, np.int32)
        voff = np.zeros(ne + 1, np.int32)
        vids = np.zeros(max(nv, 1), np.int32)
        doff = np.zeros(ne + 1, np.int64)
        data = np.zeros(max(nd, 1))
        check(self.L.spg_graph_get_edges(self.h, _p(kind, C.c_int32), _p(voff, C.c_int32), _p(vids, C.c_int32), _p(doff, C.c_int64), _p(data, C.c_double)), self.ctx.h, "get_edges")
        return {"kind": kind, "vert_off": voff, "vert_ids": vids[:nv], "data_off": doff, "data": data[:nd]}

    def blankets(self):
        n = self.L.spg_graph_last_blanket_count(self.h)
        root, rnd, status, info = (np.zeros(n, np.int32) for _ in range(4))
        kld, gap = np.zeros(n), np.zeros(n)
        self.L.spg_graph_last_blankets(self.h, _p(root, C.c_int32), _p(rnd, C.c_int32), _p(status, C.c_int32), _p(info, C.c_int32), _p(kld, C.c_double), _p(gap, C.c_double))
        return {"root": root, "round": rnd, "status": status, "info": info, "kld": kld, "min_gap": gap}

    def write(self, fname):
        check(self.L.spg_graph_write_g2o(self.h, fname.encode()), self.ctx.h, "write")

    def printStats(self):
        """nodes / edges line of src/graph_wrapper_g2o.cpp:606-612 (fill-in needs the LM Hessian: omitted)"""
        return f"nodes = {self.numVertices() - 1}; edges = {self.numEdges()}"

    def close(self):
        if getattr(self, "h", None):
            # a graph's arena belongs to its context's backend: once the context is gone (Context.close() destroys the graphs
            # it still knows first, so this only happens when finalisers run in an arbitrary order inside a reference cycle)
            # the handle must not be touched any more
            if getattr(self.ctx, "h", None):
                self.L.spg_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
