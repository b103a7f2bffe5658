// include/spg_graph_wrapper.hpp — C++ host façade over the C ABI (include/spg.h), header-only.
//
// Mirrors the reference's operator interface for the accelerated path so that its call sites
// (src/evaluate.cpp:32-221, src/compute_substitute_edge.cpp:13-96, src/test_marginalize_se3.cpp:20-48,
// src/test_marginalize_within_window.cpp:117-182, src/kld_compare.cpp) keep their shape:
//
//   reference                                          here
//   ------------------------------------------------   -----------------------------------------
//   class GraphWrapper        (src/graph_wrapper.h:17-78)   spg::GraphWrapper — the SAME virtual set:
//                                                        addVertex addEdge optimize clonePortion estimate
//                                                        information covariance marginalize write(stream)
//                                                        write(fname) kullbackLeibler chi2(other) chi2()
//                                                        vertices vertex debugPrint printStats setEstimate,
//                                                        nested Vertex {id estimate edges is2d is3d} and
//                                                        Edge {vertices measurement information}
//   class GraphWrapperG2O     (src/graph_wrapper_g2o.h:29)  spg::GraphWrapperHIP (+ marginalizeNoOptimize,
//                                                        optimizeFromId, the file constructor)
//   struct SparsityOptions    (src/sparsity_options.h:11)   spg::SparsityOptions (same fields/defaults)
//   struct DecimateOptions, globalDecimate, onlineDecimate, clusterDecimate, DecimateFunction
//                             (src/decimation.h:13-22)      identical names and signatures
//   class IsometryXd          (src/isometryxd.h:14)         spg::IsometryXd: compose / inverse / vector(mode)
//                                                        with the four SE3 modes of src/isometryxd.cpp:105-128
//   Eigen::MatrixXd / VectorXd                               spg::MatrixXd (row-major, rows() cols() (i,j) data())
//                                                        / spg::VectorXd — Eigen is not a dependency
//
// Errors: the reference asserts/aborts; this façade throws std::runtime_error with the library's
// message. Thread model: one GraphWrapperHIP per host thread (as the reference's one VertexRemover
// per call, src/vertex_remover.h:92-98). Vertex / Edge views returned by vertices() / vertex(id) are owned
// by the wrapper and stay valid until its next mutating call (the reference's views die with the g2o
// object they wrap, src/vertex_remover.cpp:518).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <fstream>
#include <memory>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>
#include "spg.h"

// ---- src/decimation.h:13-22, verbatim API -------------------------------------------------
struct DecimateOptions {
    int sparsity;
    int clusterSize;
};
inline std::vector<int> spg_decimate_call_(int (*fn)(int, int, int, int, int32_t *, int), int last, int endvert,
                                           const DecimateOptions &o) {
    std::vector<int32_t> buf((size_t)(endvert > 0 ? endvert : 0) + 8);
    int n = fn(last, endvert, o.sparsity, o.clusterSize, buf.data(), (int)buf.size());
    return std::vector<int>(buf.begin(), buf.begin() + n);
}
inline std::vector<int> clusterDecimate(int last, int endvert, const DecimateOptions &o) { return spg_decimate_call_(spg_decimate_cluster, last, endvert, o); }
inline std::vector<int> onlineDecimate(int last, int endvert, const DecimateOptions &o) { return spg_decimate_call_(spg_decimate_online, last, endvert, o); }
inline std::vector<int> globalDecimate(int last, int endvert, const DecimateOptions &o) { return spg_decimate_call_(spg_decimate_global, last, endvert, o); }
typedef std::vector<int> (*DecimateFunction)(int last, int endvert, const DecimateOptions &opts);

namespace spg {

// ---- stand-ins for Eigen::VectorXd / Eigen::MatrixXd in the signatures ---------------------------
typedef std::vector<double> VectorXd;
class MatrixXd {
public:
    MatrixXd() : _r(0), _c(0) {}
    MatrixXd(int r, int c, double fill = 0.0) : _r(r), _c(c), _a((size_t)r * c, fill) {}
    static MatrixXd Identity(int n) { MatrixXd m(n, n); for (int i = 0; i < n; i++) m(i, i) = 1.0; return m; }
    int rows() const { return _r; }
    int cols() const { return _c; }
    double &operator()(int i, int j) { return _a[(size_t)i * _c + j]; }
    double operator()(int i, int j) const { return _a[(size_t)i * _c + j]; }
    double *data() { return _a.data(); }
    const double *data() const { return _a.data(); }
    const std::vector<double> &storage() const { return _a; }   // row-major
private:
    int _r, _c;
    std::vector<double> _a;
};

// ---- src/sparsity_options.h:11-30 -----------------------------------------------------------
struct SparsityOptions {
    enum SparsityTopology { Tree, Subgraph, CliqueySubgraph, Dense, CliqueyDense };
    enum LinearizationPoint { Local, Global };
    SparsityTopology topology;
    double chordRatio;
    LinearizationPoint linPoint;
    bool includeIntraClique;
    SparsityOptions() : topology(Tree), chordRatio(1), linPoint(Local), includeIntraClique(true) {}
};

// ---- src/isometryxd.h:14-47 ----------------------------------------------------------------------
class IsometryXd {
public:
    // SE3 vector forms of src/isometryxd.h:17-22 / src/isometryxd.cpp:105-128. The two Euler forms are g2o's
    // internal::toVectorET (translation + roll, pitch, yaw) and the reference's toVectorISAM (the same with
    // components 3 and 5 swapped, src/isometryxd.cpp:131-136); g2o is an un-vendored dependency, its toEuler is
    // restated from the published definition.
    enum SE3Mode { EulerAnglesISAM, EulerAnglesG2O, CondensedQuaternion, Quaternion };

    explicit IsometryXd(bool is2d = true) : _2d(is2d) {
        if (is2d) _v = {0, 0, 0};
        else _v = {0, 0, 0, 0, 0, 0, 1};
    }
    // SE2: (x, y, theta); SE3: (tx, ty, tz, qx, qy, qz, qw) — IsometryXd::Quaternion mode
    explicit IsometryXd(const std::vector<double> &v) : _2d(v.size() == 3), _v(v) {
        if (v.size() != 3 && v.size() != 7) throw std::runtime_error("IsometryXd: need 3 (SE2) or 7 (SE3, t+quat) numbers");
        if (!_2d) {
            double n = std::sqrt(_v[3] * _v[3] + _v[4] * _v[4] + _v[5] * _v[5] + _v[6] * _v[6]);
            for (int i = 3; i < 7; i++) _v[i] /= n;
        }
    }
    bool is2d() const { return _2d; }
    bool is3d() const { return !_2d; }
    // storage form: SE2 (x y theta), SE3 (t, unit quaternion) = vector(Quaternion)
    const std::vector<double> &vector() const { return _v; }
    VectorXd vector(SE3Mode mode) const {
        if (_2d || mode == Quaternion) return _v;
        double qx = _v[3], qy = _v[4], qz = _v[5], qw = _v[6];
        if (mode == CondensedQuaternion) {   // g2o toVectorMQT: t + (qx qy qz) of the quaternion with w >= 0
            double s = qw < 0 ? -1.0 : 1.0;
            return VectorXd{_v[0], _v[1], _v[2], s * qx, s * qy, s * qz};
        }
        double roll = std::atan2(2 * (qw * qx + qy * qz), 1 - 2 * (qx * qx + qy * qy));
        double sp = 2 * (qw * qy - qz * qx);
        double pitch = std::asin(sp > 1 ? 1 : (sp < -1 ? -1 : sp));
        double yaw = std::atan2(2 * (qw * qz + qx * qy), 1 - 2 * (qy * qy + qz * qz));
        if (mode == EulerAnglesG2O) return VectorXd{_v[0], _v[1], _v[2], roll, pitch, yaw};
        return VectorXd{_v[0], _v[1], _v[2], yaw, pitch, roll};   // EulerAnglesISAM
    }

    IsometryXd inverse() const {
        if (_2d) {
            double c = std::cos(_v[2]), s = std::sin(_v[2]);
            return IsometryXd(std::vector<double>{-(c * _v[0] + s * _v[1]), -(-s * _v[0] + c * _v[1]), wrap(-_v[2])});
        }
        double q[4] = {-_v[3], -_v[4], -_v[5], _v[6]}, t[3];
        rot(q, &_v[0], t);
        return IsometryXd(std::vector<double>{-t[0], -t[1], -t[2], q[0], q[1], q[2], q[3]});
    }
    IsometryXd operator*(const IsometryXd &o) const {
        if (_2d != o._2d) throw std::runtime_error("Incompatible product");
        if (_2d) {
            double c = std::cos(_v[2]), s = std::sin(_v[2]);
            return IsometryXd(std::vector<double>{_v[0] + c * o._v[0] - s * o._v[1], _v[1] + s * o._v[0] + c * o._v[1], wrap(_v[2] + o._v[2])});
        }
        double t[3], q[4];
        rot(&_v[3], &o._v[0], t);
        const double *a = &_v[3], *b = &o._v[3];
        q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
        q[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
        q[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
        q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
        return IsometryXd(std::vector<double>{_v[0] + t[0], _v[1] + t[1], _v[2] + t[2], q[0], q[1], q[2], q[3]});
    }
    IsometryXd &operator*=(const IsometryXd &o) { return (*this) = (*this) * o; }

private:
    static double wrap(double th) {
        const double PI = 3.14159265358979323846;
        if (th >= -PI && th < PI) return th;
        double m = std::fmod(th, 2 * PI);
        if (m >= PI) m -= 2 * PI;
        if (m < -PI) m += 2 * PI;
        return m;
    }
    static void rot(const double *q, const double *v, double *out) {  // out = R(q) v
        double x = q[0], y = q[1], z = q[2], w = q[3];
        double tx = 2 * (y * v[2] - z * v[1]), ty = 2 * (z * v[0] - x * v[2]), tz = 2 * (x * v[1] - y * v[0]);
        out[0] = v[0] + w * tx + (y * tz - z * ty);
        out[1] = v[1] + w * ty + (z * tx - x * tz);
        out[2] = v[2] + w * tz + (x * ty - y * tx);
    }
    bool _2d;
    std::vector<double> _v;
};

// ---- src/graph_wrapper.h:17-78: the full virtual set ------------------------------------------------
class GraphWrapper {
public: /* Types */
    class Edge;
    class Vertex {
    public:
        virtual ~Vertex() {}
        virtual int id() const = 0;
        virtual IsometryXd estimate() const = 0;
        virtual std::vector<const Edge *> edges() const = 0;
        virtual bool is2d() const = 0;
        virtual bool is3d() const { return !is2d(); }
    };
    class Edge {
    public:
        virtual ~Edge() {}
        virtual std::vector<const Vertex *> vertices() const = 0;
        virtual IsometryXd measurement() const = 0;
        virtual MatrixXd information() const = 0;
    };

public: /* Methods */
    virtual ~GraphWrapper() {}
    virtual void addVertex(int id, const IsometryXd &init) = 0;
    virtual void addEdge(int from, int to, const IsometryXd &meas, const MatrixXd &info) = 0;
    virtual void optimize() = 0;
    virtual GraphWrapper *clonePortion(int maxid) = 0;
    virtual VectorXd estimate() = 0;
    virtual MatrixXd information() = 0;
    virtual MatrixXd covariance() = 0;
    virtual void marginalize(const std::vector<int> &which, const SparsityOptions &options) = 0;
    virtual void write(std::ostream &s) = 0;
    virtual void write(const char *fname) { std::ofstream f(fname); write(f); f.close(); }
    virtual double kullbackLeibler(GraphWrapper *other) = 0;
    virtual double chi2(GraphWrapper *other) = 0;
    virtual double chi2() const = 0;
    virtual const std::vector<Vertex *> &vertices() const = 0;
    virtual Vertex *vertex(int id) = 0;
    virtual void debugPrint(std::ostream &s) const = 0;
    virtual void printStats(std::ostream &s) const = 0;
    virtual void setEstimate(int vertexid, const IsometryXd &est) = 0;
};
inline std::ostream &operator<<(std::ostream &s, const GraphWrapper &gw) { gw.debugPrint(s); return s; }

// ---- GraphWrapperG2O (src/graph_wrapper_g2o.h:29-156) on the MI355X ---------------------------------
class GraphWrapperHIP : public GraphWrapper {
    struct Ctx {
        spg_ctx *h = nullptr;
        ~Ctx() { if (h) spg_ctx_destroy(h); }
    };
    class EdgeView;
    class VertexView : public GraphWrapper::Vertex {
    public:
        int id() const override { return _id; }
        IsometryXd estimate() const override { return _est; }
        std::vector<const GraphWrapper::Edge *> edges() const override { return _edges; }
        bool is2d() const override { return _est.is2d(); }
        int _id = 0;
        IsometryXd _est;
        std::vector<const GraphWrapper::Edge *> _edges;
    };
    class EdgeView : public GraphWrapper::Edge {
    public:
        std::vector<const GraphWrapper::Vertex *> vertices() const override { return _verts; }
        // pose-pose edge: its measurement; n-ary GLC edge: the reparametrised measurement has no IsometryXd form
        IsometryXd measurement() const override {
            if (_kind != SPG_EDGE_BINARY) throw std::runtime_error("measurement(): n-ary edge (GLC / MultiEdgeCorrelated: use record())");
            return IsometryXd(std::vector<double>(_rec.begin(), _rec.begin() + (_d == 3 ? 3 : 7)));
        }
        // pose-pose edge: d x d; GLC edge: I_r (src/topology_provider_glc.cpp:91)
        MatrixXd information() const override {
            if (_kind == SPG_EDGE_MULTI) {   // MultiEdgeCorrelated: the joint information W^T W of its nm measurements (include/spg.h)
                const int nm = (int)_rec[0], r = _d * nm;
                const double *W = _rec.data() + 1 + 2 * nm + nm * (_d == 3 ? 3 : 7);
                MatrixXd m(r, r);
                for (int i = 0; i < r; i++) for (int j = 0; j < r; j++) { double v = 0; for (int t = 0; t < r; t++) v += W[t * r + i] * W[t * r + j]; m(i, j) = v; }
                return m;
            }
            if (_kind != SPG_EDGE_BINARY) { int n = _d * (int)_verts.size(); return MatrixXd::Identity(((int)_rec.size() - n) / n); }
            MatrixXd m(_d, _d);
            int ps = _d == 3 ? 3 : 7, p = 0;
            for (int i = 0; i < _d; i++) for (int j = i; j < _d; j++) { m(i, j) = m(j, i) = _rec[ps + p]; p++; }
            return m;
        }
        int kind() const { return _kind; }
        const std::vector<double> &record() const { return _rec; }   // as in spg_batch.edge_data
        int _kind = 0, _d = 3;
        std::vector<double> _rec;
        std::vector<const GraphWrapper::Vertex *> _verts;
    };

public:
    // GraphWrapperG2O(verbose, useGLC) (src/graph_wrapper_g2o.cpp:102)
    explicit GraphWrapperHIP(int pose_dim, bool useGLC = false, int device = 0) : _ctx(std::make_shared<Ctx>()), _glc(useGLC) {
        check(spg_ctx_create(&_ctx->h, device), "spg_ctx_create (no gfx950 device? there is no CPU fallback)");
        check(spg_graph_create(_ctx->h, pose_dim, &_g), "spg_graph_create");
    }
    // GraphWrapperG2O(fname, optimize, useGLC) (src/graph_wrapper_g2o.cpp:107-154)
    GraphWrapperHIP(const char *fname, bool optimizeAtLoad = false, bool useGLC = false, int device = 0) : _ctx(std::make_shared<Ctx>()), _glc(useGLC) {
        check(spg_ctx_create(&_ctx->h, device), "spg_ctx_create (no gfx950 device? there is no CPU fallback)");
        check(spg_graph_load_g2o(_ctx->h, fname, &_g), "spg_graph_load_g2o");
        if (optimizeAtLoad) optimize();
    }
    // dense / block-sparse factorisation behind optimize() and kullbackLeibler() of this wrapper's context (SPG_SOLVER_AUTO by
    // default: by size) — CHOLMOD's / SimplicialLLT's role in src/graph_wrapper_g2o.cpp:250-269,531-548
    // arena capacity up front + the host-side buffers of a marginalisation sized and touched (include/spg.h: spg_graph_reserve)
    void reserve(long long arena_doubles) { check(spg_graph_reserve(_g, arena_doubles), "spg_graph_reserve"); }
    enum LinearSolver { SolverAuto = SPG_SOLVER_AUTO, SolverDense = SPG_SOLVER_DENSE, SolverSparse = SPG_SOLVER_SPARSE, SolverPCG = SPG_SOLVER_PCG };
    void setLinearSolver(int solver) { check(spg_ctx_set_linear_solver(_ctx->h, solver), "spg_ctx_set_linear_solver"); }
    // SolverPCG: tolerance on ||r|| / ||b|| and iteration cap of each solve (<= 0: defaults); counters of the last optimize()
    void setPcg(double rel_tol, int max_iter) { check(spg_ctx_set_pcg(_ctx->h, rel_tol, max_iter), "spg_ctx_set_pcg"); }
    // Stop rule of the factor descent (setFactorDescent; spg_ctx_set_factor_descent in include/spg.h): <= 0 = the defaults,
    // rel_tol == 0 with max_cycles > 0 = exactly that many cycles
    void setFactorDescentParams(double rel_tol, int max_cycles) { check(spg_ctx_set_factor_descent(_ctx->h, rel_tol, max_cycles), "spg_ctx_set_factor_descent"); }
    spg_pcg_stats pcgStats() const { spg_pcg_stats st{}; check(spg_ctx_pcg_stats(_ctx->h, &st), "spg_ctx_pcg_stats"); return st; }
    // How selectCandidates / pruneCandidates / pruneEdges of this wrapper's context get at Sigma (spg_ctx_set_greedy_method
    // in include/spg.h): the joint block of all endpoints (default, at most 46 000 variables), covariance columns solved
    // round by round (no bound), or JOINT where it fits and LAZY beyond. lookahead: candidates per panel, 0 = a full panel.
    enum GreedyMethod { GreedyJoint = SPG_GREEDY_JOINT, GreedyLazy = SPG_GREEDY_LAZY, GreedyAuto = SPG_GREEDY_AUTO };
    void setGreedyMethod(int method, int lookahead = 0) { check(spg_ctx_set_greedy_method(_ctx->h, method, lookahead), "spg_ctx_set_greedy_method"); }
    spg_greedy_stats greedyStats() const { spg_greedy_stats st{}; check(spg_ctx_greedy_stats(_ctx->h, &st), "spg_ctx_greedy_stats"); return st; }
    GraphWrapperHIP(const GraphWrapperHIP &) = delete;
    GraphWrapperHIP &operator=(const GraphWrapperHIP &) = delete;
    ~GraphWrapperHIP() override {
        drop_views();
        if (_g) spg_graph_destroy(_g);
    }

    void addVertex(int id, const IsometryXd &init) override { drop_views(); check(spg_graph_add_vertex(_g, id, init.vector().data()), "addVertex"); }
    void addEdge(int from, int to, const IsometryXd &meas, const MatrixXd &info) override {
        int d = spg_graph_pose_dim(_g);
        if (info.rows() != d || info.cols() != d) throw std::runtime_error("addEdge: information must be d x d");
        std::vector<double> up;
        for (int i = 0; i < d; i++) for (int j = i; j < d; j++) up.push_back(info(i, j));
        drop_views();
        check(spg_graph_add_edge(_g, from, to, meas.vector().data(), up.data()), "addEdge");
    }
    // convenience: information as d*d row-major numbers
    void addEdge(int from, int to, const IsometryXd &meas, const std::vector<double> &info) {
        int d = spg_graph_pose_dim(_g);
        if ((int)info.size() != d * d) throw std::runtime_error("addEdge: information must be d*d row-major");
        MatrixXd m(d, d);
        std::copy(info.begin(), info.end(), m.data());
        addEdge(from, to, meas, m);
    }
    // GraphWrapperG2O::optimize (src/graph_wrapper_g2o.cpp:250-269): the smallest-id vertex fixed, g2o LM x 50
    void optimize() override { optimizeFromId(-1); }
    // GraphWrapperG2O::optimizeFromId (src/graph_wrapper_g2o.cpp:271-289): the given vertex fixed
    spg_optimize_stats optimizeFromId(int first_vertex_id, int iterations = 50) {
        spg_optimize_stats st;
        drop_views();
        check(spg_graph_optimize(_g, iterations, first_vertex_id, &st), "optimize");
        _last_opt = st;
        return st;
    }
    const spg_optimize_stats &lastOptimize() const { return _last_opt; }
    // Initial estimates from the measurements alone, the step before optimize() for a graph with poor stored poses
    // (include/spg.h at spg_graph_initialize): SPG_INIT_CHORDAL on the device, SPG_INIT_SPANNING_TREE on the host (g2o's
    // computeInitialGuess). The fixed vertex (fixed_id < 0: the smallest id) keeps its pose.
    spg_init_stats initialize(int method = SPG_INIT_CHORDAL, int fixed_id = -1) {
        spg_init_stats st;
        drop_views();
        check(spg_graph_initialize(_g, method, fixed_id, &st), "initialize");
        return st;
    }
    // g2o's setRobustKernel for optimize() / chi2(other) (include/spg.h at spg_graph_set_robust_kernel): SPG_ROBUST_* of
    // width delta on the binary edges whose vertex ids are at least minIdGap apart. chi2(), information(), the covariances,
    // the KLDs and the marginalisation never see it; clear it (SPG_ROBUST_NONE) before optimising a sparsified graph.
    void setRobustKernel(int kind, double delta = 1.0, int minIdGap = 1) { check(spg_graph_set_robust_kernel(_g, kind, delta, minIdGap), "setRobustKernel"); }
    struct RobustKernel { int kind; double delta; int minIdGap; };
    RobustKernel robustKernel() const {
        RobustKernel k{};
        check(spg_graph_get_robust_kernel(_g, &k.kind, &k.delta, &k.minIdGap), "robustKernel");
        return k;
    }
    // per edge, in the order of edges(), at the stored estimates: the plain chi2, and rho / weight of the robust kernel
    struct EdgeChi2 { std::vector<double> chi2, rho, weight; };
    EdgeChi2 edgeChi2() const {
        EdgeChi2 out;
        const int n = spg_graph_edge_chi2(_g, nullptr, nullptr, nullptr, 0);
        check(std::min(n, 0), "edgeChi2");
        out.chi2.resize((size_t)n); out.rho.resize((size_t)n); out.weight.resize((size_t)n);
        check(std::min(spg_graph_edge_chi2(_g, out.chi2.data(), out.rho.data(), out.weight.data(), n), 0), "edgeChi2");
        return out;
    }
    // GraphWrapperG2O::clonePortion (src/graph_wrapper_g2o.cpp:334-356): vertices / edges up to maxid, optimised
    GraphWrapperHIP *clonePortion(int maxid) override {
        spg_graph *c = nullptr;
        check(spg_graph_clone_portion(_g, maxid, &c), "clonePortion");
        GraphWrapperHIP *gw = new GraphWrapperHIP(_ctx, c, _glc);
        if (spg_graph_num_vertices(c) > 1 && spg_graph_num_edges(c) > 0) gw->optimize();
        return gw;
    }
    // GraphWrapperG2O::estimate (src/graph_wrapper_g2o.cpp:358-361) = stack() (src/utils.cpp:200-221): every vertex
    // but the first, id order, SE2 (x y theta) / SE3 toVectorISAM
    VectorXd estimate() override {
        VectorXd out;
        const std::vector<Vertex *> &vs = vertices();
        for (size_t i = 1; i < vs.size(); i++) {
            VectorXd v = vs[i]->estimate().vector(IsometryXd::EulerAnglesISAM);
            out.insert(out.end(), v.begin(), v.end());
        }
        return out;
    }
    // GraphWrapperG2O::information (src/graph_wrapper_g2o.cpp:363-366): n x n, first vertex fixed
    MatrixXd information() override {
        int64_t n = spg_graph_information(_g, -1, nullptr, 0);
        check((int)std::min<int64_t>(n, 0), "information");
        MatrixXd H((int)n, (int)n);
        check((int)std::min<int64_t>(spg_graph_information(_g, -1, H.data(), n * n), 0), "information");
        return H;
    }
    // GraphWrapperG2O::sparseInformation (src/graph_wrapper_g2o.cpp:382-396): information() in block-CSR form at any size.
    // D x D row-major blocks, both triangles, columns ascending within a row; ids names the block rows (ascending).
    struct BlockCSR {
        int blockDim = 0;
        std::vector<int64_t> rowPtr;     // rows() + 1
        std::vector<int32_t> colIdx;     // blocks()
        std::vector<double> values;      // blocks() * blockDim^2; empty for a pattern-only export
        std::vector<int32_t> ids;        // vertex id of each block row
        int rows() const { return (int)ids.size(); }
        int64_t blocks() const { return (int64_t)colIdx.size(); }
    };
    void sparseInformation(BlockCSR &out, int fixed_id = -1, bool values = true) {
        const int d = spg_graph_pose_dim(_g);
        const int64_t nnzb = spg_graph_sparse_information(_g, fixed_id, nullptr, nullptr, nullptr, 0, nullptr);
        check((int)std::min<int64_t>(nnzb, 0), "sparseInformation");
        const int nb = std::max(spg_graph_num_vertices(_g) - 1, 0);
        out.blockDim = d;
        out.rowPtr.assign((size_t)nb + 1, 0);
        out.colIdx.assign((size_t)nnzb, 0);
        out.values.assign(values ? (size_t)nnzb * d * d : 0, 0.0);
        out.ids.assign((size_t)nb, 0);
        std::vector<int32_t> col((size_t)std::max<int64_t>(nnzb, 1));
        std::vector<double> val(values ? (size_t)std::max<int64_t>(nnzb, 1) * d * d : 0);
        std::vector<int32_t> ids((size_t)std::max(nb, 1));
        check((int)std::min<int64_t>(spg_graph_sparse_information(_g, fixed_id, out.rowPtr.data(), col.data(), values ? val.data() : nullptr, nnzb, ids.data()), 0),
              "sparseInformation");
        std::copy(col.begin(), col.begin() + nnzb, out.colIdx.begin());
        std::copy(val.begin(), val.begin() + out.values.size(), out.values.begin());
        std::copy(ids.begin(), ids.begin() + nb, out.ids.begin());
    }
    // Y = information() * X without forming the matrix densely; X holds nrhs vectors of length d * (vertices - 1), one
    // after the other, and so does the result
    std::vector<double> informationApply(const std::vector<double> &X, int nrhs = 1, int fixed_id = -1) {
        const size_t n = (size_t)spg_graph_pose_dim(_g) * (size_t)std::max(spg_graph_num_vertices(_g) - 1, 0);
        if (nrhs <= 0 || X.size() != n * (size_t)nrhs) throw std::runtime_error("informationApply: X must hold nrhs vectors of d * (vertices - 1) numbers");
        std::vector<double> Y(X.size(), 0.0);
        if (n > 0) check(spg_graph_information_apply(_g, fixed_id, X.data(), nrhs, Y.data()), "informationApply");
        return Y;
    }
    // GraphWrapperG2O::covariance (src/graph_wrapper_g2o.cpp:368-373)
    MatrixXd covariance() override {
        int64_t n = spg_graph_covariance(_g, -1, nullptr, 0);
        check((int)std::min<int64_t>(n, 0), "covariance");
        MatrixXd S((int)n, (int)n);
        check((int)std::min<int64_t>(spg_graph_covariance(_g, -1, S.data(), n * n), 0), "covariance");
        return S;
    }
    // GraphWrapperG2O::marginalizeNoOptimize (src/graph_wrapper_g2o.cpp:398-453)
    void marginalizeNoOptimize(const std::vector<int> &which, const SparsityOptions &o) {
        spg_options so;
        so.pose_dim = spg_graph_pose_dim(_g);
        so.algorithm = _glc ? SPG_ALG_GLC : SPG_ALG_NFR;
        so.topology = (int)o.topology;
        so.lin_point = (int)o.linPoint;
        so.include_intra_clique = o.includeIntraClique ? 1 : 0;
        so.flags = ((_glc && _glc_kld) ? SPG_FLAG_GLC_KLD : 0) | ((!_glc && _factor_descent) ? SPG_FLAG_NFR_FACTOR_DESCENT : 0);
        so.chord_ratio = o.chordRatio;
        std::vector<int32_t> w(which.begin(), which.end());
        drop_views();
        check(spg_graph_marginalize(_g, w.data(), (int)w.size(), &so, &_stats), "marginalize");
    }
    // GraphWrapperG2O::marginalize (src/graph_wrapper_g2o.cpp:455-463): marginalizeNoOptimize + optimize()
    void marginalize(const std::vector<int> &which, const SparsityOptions &o) override {
        marginalizeNoOptimize(which, o);
        optimize();
    }
    // GraphWrapper::write (src/graph_wrapper.h:62-64, src/graph_wrapper_g2o.cpp:467-470)
    void write(std::ostream &s) override {
        char *text = nullptr;
        size_t len = 0;
        check(spg_graph_write_g2o_mem(_g, &text, &len), "write");
        s.write(text, (std::streamsize)len);
        spg_free(text);
    }
    void write(const char *fname) override { check(spg_graph_write_g2o(_g, fname), "write"); }
    // GraphWrapperG2O::kullbackLeibler(other), called on the baseline (src/graph_wrapper_g2o.cpp:531-548)
    double kullbackLeibler(GraphWrapper *other) override { return kullbackLeibler(other, nullptr); }
    double kullbackLeibler(GraphWrapper *other, spg_kld_terms *terms) {
        GraphWrapperHIP *o = dynamic_cast<GraphWrapperHIP *>(other);
        if (!o) throw std::runtime_error("kullbackLeibler: the other graph is not a GraphWrapperHIP");
        spg_kld_terms t;
        check(spg_graph_kullback_leibler(_g, o->_g, -1, &t), "kullbackLeibler");
        if (terms) *terms = t;
        return t.kld;
    }
    // GraphWrapperISAM::covariance (src/graph_wrapper_isam.cpp:259-262, covariances().marginal): the D x D marginal
    // covariance of each vertex of `ids` (empty: every vertex, ascending id), read from the sparse factor's selected
    // inverse; one d x d matrix per vertex, the fixed vertex's is zero. Not part of the reference's virtual set.
    std::vector<MatrixXd> marginalCovariances(const std::vector<int> &ids = {}, int fixed_id = -1, spg_cov_stats *stats = nullptr) {
        const int d = spg_graph_pose_dim(_g);
        std::vector<int32_t> w(ids.begin(), ids.end());
        const int32_t *wp = ids.empty() ? nullptr : w.data();
        int64_t need = spg_graph_marginal_covariances(_g, fixed_id, wp, (int)w.size(), nullptr, 0, nullptr);
        check((int)std::min<int64_t>(need, 0), "marginalCovariances");
        std::vector<double> buf((size_t)std::max<int64_t>(need, 1));
        check((int)std::min<int64_t>(spg_graph_marginal_covariances(_g, fixed_id, wp, (int)w.size(), buf.data(), need, stats), 0), "marginalCovariances");
        return split_blocks(buf, need / (d * d), d);
    }
    // the 2D x 2D covariance [[Saa, Sab], [Sba, Sbb]] of each pair of vertices that share a live edge
    std::vector<MatrixXd> jointCovariances(const std::vector<std::pair<int, int>> &pairs, int fixed_id = -1, spg_cov_stats *stats = nullptr) {
        const int d = spg_graph_pose_dim(_g);
        std::vector<int32_t> p;
        for (auto &q : pairs) { p.push_back(q.first); p.push_back(q.second); }
        int64_t need = spg_graph_joint_covariances(_g, fixed_id, p.data(), (int)pairs.size(), nullptr, 0, nullptr);
        check((int)std::min<int64_t>(need, 0), "jointCovariances");
        std::vector<double> buf((size_t)std::max<int64_t>(need, 1));
        check((int)std::min<int64_t>(spg_graph_joint_covariances(_g, fixed_id, p.data(), (int)pairs.size(), buf.data(), need, stats), 0), "jointCovariances");
        return split_blocks(buf, (int64_t)pairs.size(), 2 * d);
    }
    // the 2D x 2D covariance [[Saa, Sab], [Sba, Sbb]] of each pair of distinct vertices, with or without a common edge
    std::vector<MatrixXd> pairCovariances(const std::vector<std::pair<int, int>> &pairs, int fixed_id = -1, spg_cov_solve_stats *stats = nullptr) {
        const int d = spg_graph_pose_dim(_g);
        std::vector<int32_t> p;
        for (auto &q : pairs) { p.push_back(q.first); p.push_back(q.second); }
        int64_t need = spg_graph_pair_covariances(_g, fixed_id, p.data(), (int)pairs.size(), nullptr, 0, nullptr);
        check((int)std::min<int64_t>(need, 0), "pairCovariances");
        std::vector<double> buf((size_t)std::max<int64_t>(need, 1));
        check((int)std::min<int64_t>(spg_graph_pair_covariances(_g, fixed_id, p.data(), (int)pairs.size(), buf.data(), need, stats), 0), "pairCovariances");
        return split_blocks(buf, (int64_t)pairs.size(), 2 * d);
    }
    // GraphWrapperISAM::covariance (src/graph_wrapper_isam.cpp:259-262): the (nD) x (nD) joint covariance of the listed
    // vertices in the order given, off-diagonal blocks mirrored exactly
    MatrixXd jointMarginalCovariance(const std::vector<int> &ids, int fixed_id = -1, spg_cov_solve_stats *stats = nullptr) {
        const int d = spg_graph_pose_dim(_g);
        std::vector<int32_t> w(ids.begin(), ids.end());
        int64_t need = spg_graph_joint_marginal_covariance(_g, fixed_id, w.data(), (int)w.size(), nullptr, 0, nullptr);
        check((int)std::min<int64_t>(need, 0), "jointMarginalCovariance");
        std::vector<double> buf((size_t)std::max<int64_t>(need, 1));
        check((int)std::min<int64_t>(spg_graph_joint_marginal_covariance(_g, fixed_id, w.data(), (int)w.size(), buf.data(), need, stats), 0),
              "jointMarginalCovariance");
        return split_blocks(buf, 1, (int)w.size() * d)[0];
    }
    // the relative pose Xa^-1 Xb of each pair of distinct vertices (the numbers of IsometryXd::vector(), exactly as the
    // device wrote them) and its D x D covariance P = J Sigma_ab J^T (include/spg.h: spg_graph_relative_covariances);
    // addEdge(a, b, IsometryXd(first), inverse of second) is the marginal relative-pose factor of the pair
    std::vector<std::pair<VectorXd, MatrixXd>> relativeCovariances(const std::vector<std::pair<int, int>> &pairs, int fixed_id = -1,
                                                                     spg_cov_solve_stats *stats = nullptr) {
        const int d = spg_graph_pose_dim(_g), ps = d == 3 ? 3 : 7;
        std::vector<int32_t> p;
        for (auto &q : pairs) { p.push_back(q.first); p.push_back(q.second); }
        int64_t need = spg_graph_relative_covariances(_g, fixed_id, p.data(), (int)pairs.size(), nullptr, nullptr, 0, nullptr);
        check((int)std::min<int64_t>(need, 0), "relativeCovariances");
        std::vector<double> rel(std::max<size_t>(pairs.size(), 1) * ps), buf((size_t)std::max<int64_t>(need, 1));
        check((int)std::min<int64_t>(spg_graph_relative_covariances(_g, fixed_id, p.data(), (int)pairs.size(), rel.data(), buf.data(), need, stats), 0),
              "relativeCovariances");
        std::vector<MatrixXd> P = split_blocks(buf, (int64_t)pairs.size(), d);
        std::vector<std::pair<VectorXd, MatrixXd>> out;
        for (size_t i = 0; i < pairs.size(); i++) out.emplace_back(VectorXd(rel.begin() + i * ps, rel.begin() + (i + 1) * ps), P[i]);
        return out;
    }
    // A hypothetical binary edge and what the graph says about it (include/spg.h: spg_graph_score_candidates)
    struct Candidate {
        int from, to;
        VectorXd measurement;     // SE2 (x y theta), SE3 (t, unit quaternion): IsometryXd::vector(), taken as given
        MatrixXd information;     // d x d
    };
    struct CandidateScore {
        double d2;      // innovation Mahalanobis distance e^T (P + Omega^-1)^-1 e: chi^2 with d degrees of freedom for an inlier
        double gain;    // information gain 1/2 ln det(I + Omega P), nats
        double chi2;    // e^T Omega e
        int status;     // SPG_CAND_SCORED, or SPG_CAND_INFO_NOT_PD (the three values are NaN)
    };
    std::vector<CandidateScore> scoreCandidates(const std::vector<Candidate> &cands, int fixed_id = -1, spg_cov_solve_stats *stats = nullptr) {
        const int d = spg_graph_pose_dim(_g), n = (int)cands.size();
        std::vector<int32_t> ij;
        std::vector<double> rec;
        for (const Candidate &c : cands) {
            if (c.information.rows() != d || c.information.cols() != d) throw std::runtime_error("scoreCandidates: information must be d x d");
            const VectorXd &z = c.measurement;
            if ((int)z.size() != (d == 3 ? 3 : 7)) throw std::runtime_error("scoreCandidates: the measurement does not match the graph's pose dimension");
            ij.push_back(c.from); ij.push_back(c.to);
            rec.insert(rec.end(), z.begin(), z.end());
            for (int i = 0; i < d; i++) for (int j = i; j < d; j++) rec.push_back(c.information(i, j));
        }
        std::vector<double> d2((size_t)std::max(n, 1)), gain(d2.size()), chi2(d2.size());
        std::vector<int32_t> status(d2.size());
        check(std::min(spg_graph_score_candidates(_g, fixed_id, ij.data(), rec.data(), n, d2.data(), gain.data(), chi2.data(), status.data(), n, stats), 0),
              "scoreCandidates");
        std::vector<CandidateScore> out;
        for (int i = 0; i < n; i++) out.push_back({d2[i], gain[i], chi2[i], (int)status[i]});
        return out;
    }
    // Greedy choice of up to k candidates by conditional information gain (include/spg.h: spg_graph_select_candidates):
    // (index into cands, its gain given the ones chosen before it), in order of selection. max_d2 > 0 gates on the d2 of
    // scoreCandidates, evaluated once on the graph as it stands. status, if given: SPG_CAND_* per candidate.
    std::vector<std::pair<int, double>> selectCandidates(const std::vector<Candidate> &cands, int k, double min_gain = 0.0, double max_d2 = 0.0,
                                                         int fixed_id = -1, std::vector<int> *status = nullptr, spg_select_stats *stats = nullptr) {
        const int d = spg_graph_pose_dim(_g), n = (int)cands.size();
        std::vector<int32_t> ij;
        std::vector<double> rec;
        for (const Candidate &c : cands) {
            if (c.information.rows() != d || c.information.cols() != d) throw std::runtime_error("selectCandidates: information must be d x d");
            const VectorXd &z = c.measurement;
            if ((int)z.size() != (d == 3 ? 3 : 7)) throw std::runtime_error("selectCandidates: the measurement does not match the graph's pose dimension");
            ij.push_back(c.from); ij.push_back(c.to);
            rec.insert(rec.end(), z.begin(), z.end());
            for (int i = 0; i < d; i++) for (int j = i; j < d; j++) rec.push_back(c.information(i, j));
        }
        const int cap = std::max(std::min(k, n), 0);
        std::vector<int32_t> sel((size_t)std::max(cap, 1)), st((size_t)std::max(n, 1));
        std::vector<double> gain(sel.size());
        const int r = spg_graph_select_candidates(_g, fixed_id, ij.data(), rec.data(), n, k, min_gain, max_d2, sel.data(), gain.data(), cap, nullptr,
                                                  st.data(), stats);
        check(std::min(r, 0), "selectCandidates");
        std::vector<std::pair<int, double>> out;
        for (int i = 0; i < r; i++) out.emplace_back((int)sel[i], gain[i]);
        if (status) status->assign(st.begin(), st.begin() + n);
        return out;
    }
    // Which candidates agree with each other (include/spg.h: spg_graph_compatible_candidates): the pairwise joint test at
    // pair_max_d2, the largest consistent set, then the sequential joint gate (member p + 1 against joint_max_d2[p]; an empty
    // vector: no joint gate) until k are accepted. max_d2 > 0 gates each candidate alone first. The graph is not modified.
    struct CompatResult {
        std::vector<int> compatible;      // indices into cands, in order of acceptance
        std::vector<double> joint_d2;     // the joint distance after each acceptance
        std::vector<int> clique;          // the consistent set, in order of construction
        std::vector<double> d2;           // per candidate
        std::vector<int> degree, status;  // per candidate: neighbours in the consistency graph, SPG_CAND_*
    };
    CompatResult compatibleCandidates(const std::vector<Candidate> &cands, int k, double max_d2, double pair_max_d2,
                                      const std::vector<double> &joint_max_d2 = {}, int fixed_id = -1, spg_compat_stats *stats = nullptr) {
        const int d = spg_graph_pose_dim(_g), n = (int)cands.size();
        std::vector<int32_t> ij;
        std::vector<double> rec;
        for (const Candidate &c : cands) {
            if (c.information.rows() != d || c.information.cols() != d) throw std::runtime_error("compatibleCandidates: information must be d x d");
            const VectorXd &z = c.measurement;
            if ((int)z.size() != (d == 3 ? 3 : 7)) throw std::runtime_error("compatibleCandidates: the measurement does not match the graph's pose dimension");
            ij.push_back(c.from); ij.push_back(c.to);
            rec.insert(rec.end(), z.begin(), z.end());
            for (int i = 0; i < d; i++) for (int j = i; j < d; j++) rec.push_back(c.information(i, j));
        }
        const int cap = std::max(std::min(k, n), 0);
        if (!joint_max_d2.empty() && (int)joint_max_d2.size() < cap) throw std::runtime_error("compatibleCandidates: joint_max_d2 must have min(k, n) entries");
        std::vector<int32_t> sel((size_t)std::max(cap, 1)), clq((size_t)std::max(n, 1)), deg(clq.size()), st(clq.size());
        std::vector<double> jd(sel.size()), d2(clq.size());
        spg_compat_stats cs{};
        const int r = spg_graph_compatible_candidates(_g, fixed_id, ij.data(), rec.data(), n, k, max_d2, pair_max_d2,
                                                      joint_max_d2.empty() ? nullptr : joint_max_d2.data(), sel.data(), jd.data(), cap, clq.data(), n,
                                                      d2.data(), deg.data(), st.data(), nullptr, 0, &cs);
        check(std::min(r, 0), "compatibleCandidates");
        CompatResult out;
        out.compatible.assign(sel.begin(), sel.begin() + r);
        out.joint_d2.assign(jd.begin(), jd.begin() + r);
        out.clique.assign(clq.begin(), clq.begin() + std::max(cs.clique_size, 0));
        out.d2.assign(d2.begin(), d2.begin() + n);
        out.degree.assign(deg.begin(), deg.begin() + n);
        out.status.assign(st.begin(), st.begin() + n);
        if (stats) *stats = cs;
        return out;
    }
    // Loop-closure candidates by proximity and range (include/spg.h: spg_graph_propose_candidates): the pairs of live
    // vertices within search_radius of each other (rules 1 to 5 of the header), at most the max_per_vertex nearest per query
    // vertex, and with range > 0 those whose zscore = (rho - range) / sigma is <= z_max. An empty `queries`: every vertex
    // is a query. The pairs come in ascending (id_a, id_b) order. The graph is not modified.
    struct ProposeResult {
        std::vector<std::pair<int, int>> ij;
        std::vector<double> dist, angle;
        std::vector<double> sigma, zscore;   // with range > 0
        spg_propose_stats stats;
    };
    ProposeResult proposeCandidates(double search_radius, double max_angle = 0.0, int min_id_gap = 1, int max_per_vertex = 0,
                                    const std::vector<int> &queries = {}, double range = 0.0, double z_max = 2.0, int fixed_id = -1) {
        std::vector<int32_t> q(queries.begin(), queries.end());
        const int32_t *qp = q.empty() ? nullptr : q.data();
        ProposeResult out{};
        // the size from stage A alone: the gate can only drop pairs of it; before it, with an empty query list, the call
        // checks range with the other arguments and returns 0 without touching the backend
        if (range > 0.0) {
            const int32_t none = 0;
            check((int)spg_graph_propose_candidates(_g, fixed_id, search_radius, max_angle, min_id_gap, max_per_vertex, &none, 0, range, z_max, nullptr,
                                                    nullptr, nullptr, nullptr, nullptr, 0, nullptr), "proposeCandidates");
        }
        const int64_t cap = spg_graph_propose_candidates(_g, fixed_id, search_radius, max_angle, min_id_gap, max_per_vertex, qp, (int)q.size(),
                                                         range > 0.0 ? 0.0 : range, z_max, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &out.stats);
        check((int)std::min<int64_t>(cap, 0), "proposeCandidates");
        if (cap == 0) return out;
        const size_t room = (size_t)std::max<int64_t>(cap, 1);
        std::vector<int32_t> ij(2 * room);
        std::vector<double> dist(room), angle(room), sigma(room), zscore(room);
        const int64_t n = spg_graph_propose_candidates(_g, fixed_id, search_radius, max_angle, min_id_gap, max_per_vertex, qp, (int)q.size(), range, z_max,
                                                       ij.data(), dist.data(), angle.data(), sigma.data(), zscore.data(), cap, &out.stats);
        check((int)std::min<int64_t>(n, 0), "proposeCandidates");
        for (int64_t i = 0; i < n; i++) out.ij.push_back({ij[2 * i], ij[2 * i + 1]});
        out.dist.assign(dist.begin(), dist.begin() + n);
        out.angle.assign(angle.begin(), angle.begin() + n);
        if (range > 0.0) {
            out.sigma.assign(sigma.begin(), sigma.begin() + n);
            out.zscore.assign(zscore.begin(), zscore.begin() + n);
        }
        return out;
    }
    // The vertices to remove by spatial redundancy (include/spg.h: spg_graph_select_removals): one pose is kept per
    // neighbourhood of `radius` (and of max_angle when > 0), the vertices of `keep` whatever happens, among the others the
    // higher priority first (one value per live vertex in ascending-id order; empty: a hash of the id). `removed`
    // (ascending ids) goes unchanged into marginalize(). The graph is not modified.
    struct RemovalResult {
        std::vector<int> removed, representative;   // per removed vertex: its id, the kept vertex nearest to it
        std::vector<double> rep_dist;
        spg_removal_stats stats;
    };
    RemovalResult selectRemovals(double radius, double max_angle = 0.0, const std::vector<int> &keep = {}, const std::vector<double> &priority = {}) {
        std::vector<int32_t> k(keep.begin(), keep.end());
        const int32_t *kp = k.empty() ? nullptr : k.data();
        const double *pp = priority.empty() ? nullptr : priority.data();
        RemovalResult out{};
        if (!priority.empty() && (int)priority.size() != spg_graph_num_vertices(_g)) throw std::invalid_argument("selectRemovals: one priority per live vertex");
        const int64_t cap = spg_graph_select_removals(_g, radius, max_angle, kp, (int)k.size(), pp, nullptr, nullptr, nullptr, 0, &out.stats);
        check((int)std::min<int64_t>(cap, 0), "selectRemovals");
        if (cap == 0) return out;
        std::vector<int32_t> rem((size_t)cap), rep((size_t)cap);
        out.rep_dist.resize((size_t)cap);
        const int64_t n = spg_graph_select_removals(_g, radius, max_angle, kp, (int)k.size(), pp, rem.data(), rep.data(), out.rep_dist.data(), cap, &out.stats);
        check((int)std::min<int64_t>(n, 0), "selectRemovals");
        out.removed.assign(rem.begin(), rem.begin() + n);
        out.representative.assign(rep.begin(), rep.begin() + n);
        out.rep_dist.resize((size_t)n);
        return out;
    }
    // Greedy choice of up to k of the listed live binary edges (indices into the order of spg_graph_get_edges) by
    // conditional information loss (include/spg.h: spg_graph_prune_candidates); the graph is not modified.
    struct PruneResult {
        std::vector<int> pruned;          // indices into edge_idx, in order
        std::vector<double> cond_loss;    // the loss of pruned[t] when it was chosen
        std::vector<double> kld;          // the cumulative exact KLD after round t
        std::vector<double> final_loss, final_margin;   // per candidate, after the last round
        std::vector<int> status;          // SPG_PRUNE_* per candidate
    };
    PruneResult pruneCandidates(const std::vector<int> &edge_idx, int k, double max_loss = 0.0, double max_kld = 0.0, double min_margin = 0.0,
                                int fixed_id = -1, spg_prune_stats *stats = nullptr) {
        const int n = (int)edge_idx.size(), cap = std::max(std::min(k, n), 0);
        std::vector<int32_t> idx(edge_idx.begin(), edge_idx.end()), sel((size_t)std::max(cap, 1)), st((size_t)std::max(n, 1));
        std::vector<double> loss(sel.size()), kld(sel.size()), fl(st.size()), fm(st.size());
        const int r = spg_graph_prune_candidates(_g, fixed_id, idx.data(), n, k, max_loss, max_kld, min_margin, sel.data(), loss.data(), kld.data(), cap,
                                                 fl.data(), fm.data(), st.data(), stats);
        check(std::min(r, 0), "pruneCandidates");
        PruneResult out;
        out.pruned.assign(sel.begin(), sel.begin() + r);
        out.cond_loss.assign(loss.begin(), loss.begin() + r);
        out.kld.assign(kld.begin(), kld.begin() + r);
        out.final_loss.assign(fl.begin(), fl.begin() + n);
        out.final_margin.assign(fm.begin(), fm.begin() + n);
        out.status.assign(st.begin(), st.begin() + n);
        return out;
    }
    // live edges: the indices pruneCandidates / removeEdges take run over 0 .. numEdges() - 1 (the order of spg_graph_get_edges)
    int numEdges() const { return spg_graph_num_edges(_g); }
    // removes the listed live edges (any kind); the others keep their order (spg_graph_remove_edges)
    void removeEdges(const std::vector<int> &edge_idx) {
        std::vector<int32_t> idx(edge_idx.begin(), edge_idx.end());
        drop_views();
        check(spg_graph_remove_edges(_g, idx.data(), (int)idx.size()), "removeEdges");
    }
    // pruneCandidates followed by removeEdges of what it chose
    PruneResult pruneEdges(const std::vector<int> &edge_idx, int k, double max_loss = 0.0, double max_kld = 0.0, double min_margin = 0.0,
                           int fixed_id = -1, spg_prune_stats *stats = nullptr) {
        PruneResult out = pruneCandidates(edge_idx, k, max_loss, max_kld, min_margin, fixed_id, stats);
        std::vector<int> gone;
        for (int t : out.pruned) gone.push_back(edge_idx[(size_t)t]);
        removeEdges(gone);
        return out;
    }
    // Greedy data snooping over the listed live binary edges (include/spg.h: spg_graph_detect_outliers): each round flags
    // the edge with the largest leave-one-out chi^2 statistic given the ones already flagged; the graph is not modified.
    // Call optimize() first: the stored estimates are taken as the minimiser. min_stat <= 0: no threshold.
    struct OutlierResult {
        std::vector<int> flagged;         // indices into edge_idx, in order
        std::vector<double> stat;         // the statistic of flagged[t] when it was chosen
        std::vector<double> final_stat, final_margin, redundancy;   // per candidate
        std::vector<int> status;          // SPG_OUTLIER_* per candidate
    };
    OutlierResult detectOutliers(const std::vector<int> &edge_idx, int k, double min_stat = 0.0, double min_margin = 0.0, int fixed_id = -1,
                                 spg_outlier_stats *stats = nullptr) {
        const int n = (int)edge_idx.size(), cap = std::max(std::min(k, n), 0);
        std::vector<int32_t> idx(edge_idx.begin(), edge_idx.end()), sel((size_t)std::max(cap, 1)), st((size_t)std::max(n, 1));
        std::vector<double> cs(sel.size()), fs(st.size()), fm(st.size()), red(st.size());
        const int r = spg_graph_detect_outliers(_g, fixed_id, idx.data(), n, k, min_stat, min_margin, sel.data(), cs.data(), cap, fs.data(), fm.data(),
                                                red.data(), st.data(), stats);
        check(std::min(r, 0), "detectOutliers");
        OutlierResult out;
        out.flagged.assign(sel.begin(), sel.begin() + r);
        out.stat.assign(cs.begin(), cs.begin() + r);
        out.final_stat.assign(fs.begin(), fs.begin() + n);
        out.final_margin.assign(fm.begin(), fm.begin() + n);
        out.redundancy.assign(red.begin(), red.begin() + n);
        out.status.assign(st.begin(), st.begin() + n);
        return out;
    }
    // detectOutliers followed by removeEdges of what it flagged
    OutlierResult rejectOutliers(const std::vector<int> &edge_idx, int k, double min_stat = 0.0, double min_margin = 0.0, int fixed_id = -1,
                                 spg_outlier_stats *stats = nullptr) {
        OutlierResult out = detectOutliers(edge_idx, k, min_stat, min_margin, fixed_id, stats);
        std::vector<int> gone;
        for (int t : out.flagged) gone.push_back(edge_idx[(size_t)t]);
        removeEdges(gone);
        return out;
    }
    // called on the baseline: kullbackLeiblerDivergence (src/utils.cpp:70-97) of each vertex's marginal in `other` against
    // its marginal here, every vertex of `other` but the fixed one; ids ascending
    std::vector<double> marginalKullbackLeibler(GraphWrapper *other, std::vector<int> *ids = nullptr, int fixed_id = -1, spg_cov_stats *stats = nullptr) {
        GraphWrapperHIP *o = dynamic_cast<GraphWrapperHIP *>(other);
        if (!o) throw std::runtime_error("marginalKullbackLeibler: the other graph is not a GraphWrapperHIP");
        int n = spg_graph_marginal_kld(_g, o->_g, fixed_id, nullptr, nullptr, 0, nullptr);
        check(std::min(n, 0), "marginalKullbackLeibler");
        std::vector<int32_t> id((size_t)std::max(n, 1));
        std::vector<double> kld((size_t)std::max(n, 1));
        check(std::min(spg_graph_marginal_kld(_g, o->_g, fixed_id, id.data(), kld.data(), n, stats), 0), "marginalKullbackLeibler");
        id.resize((size_t)n);
        kld.resize((size_t)n);
        if (ids) ids->assign(id.begin(), id.end());
        return kld;
    }
    // GraphWrapperG2O::chi2(other) (src/graph_wrapper_g2o.cpp:503-529): push; other's vertices take other's estimates
    // and are held fixed; optimise the rest; read chi2; pop
    double chi2(GraphWrapper *other) override {
        std::vector<int32_t> ids;
        std::vector<double> saved;
        snapshot(ids, saved);
        std::vector<int32_t> fx;
        if (!ids.empty()) fx.push_back(ids[0]);   // optimize() inside keeps the first vertex fixed (:250-252)
        for (const Vertex *v : other->vertices()) {
            check(spg_graph_set_estimate(_g, v->id(), v->estimate().vector().data()), "chi2(other): the other graph holds a vertex this one lacks");
            if (ids.empty() || v->id() != ids[0]) fx.push_back(v->id());
        }
        spg_optimize_stats st;
        int rc = spg_graph_optimize_fixed(_g, 50, fx.data(), (int)fx.size(), &st);
        restore(ids, saved);
        check(rc, "chi2(other)");
        return st.chi2_final;
    }
    // _so->chi2() (src/graph_wrapper_g2o.cpp:501)
    double chi2() const override {
        double v = 0;
        check(spg_graph_chi2(_g, &v), "chi2");
        return v;
    }
    const std::vector<Vertex *> &vertices() const override { build_views(); return _vviews; }
    // GraphWrapperG2O::vertex (src/graph_wrapper_g2o.cpp:207-212): lower_bound over the id-sorted views
    Vertex *vertex(int id) override {
        build_views();
        auto it = std::lower_bound(_vviews.begin(), _vviews.end(), id, [](const Vertex *v, int i) { return v->id() < i; });
        return (it != _vviews.end() && (*it)->id() == id) ? *it : nullptr;
    }
    // GraphWrapperG2O::debugPrint (src/graph_wrapper_g2o.cpp:577-594)
    void debugPrint(std::ostream &s) const override {
        build_views();
        s << "+ vertices: ";
        for (const Vertex *v : _vviews) s << v->id() << " ";
        s << "\n+ edges: ";
        for (const EdgeView *e : _eviews) {
            s << "(";
            for (size_t i = 0; i < e->_verts.size(); i++) s << e->_verts[i]->id() << (i + 1 < e->_verts.size() ? "," : "");
            s << ") ";
        }
        s << std::endl;
    }
    // GraphWrapperG2O::printStats (src/graph_wrapper_g2o.cpp:606-612): nodes, edges and the fill-in of the
    // information matrix (block pattern: a vertex pair is filled when some edge joins it)
    void printStats(std::ostream &s) const override {
        build_views();
        const int d = spg_graph_pose_dim(_g);
        const double nfree = (double)_vviews.size() - 1;
        std::vector<std::pair<int, int>> blocks;
        const int first = _vviews.empty() ? -1 : _vviews[0]->id();
        for (const Vertex *v : _vviews) if (v->id() != first) blocks.push_back({v->id(), v->id()});
        for (const EdgeView *e : _eviews)
            for (const Vertex *a : e->_verts) for (const Vertex *b : e->_verts)
                if (a->id() != first && b->id() != first && a->id() != b->id()) blocks.push_back({a->id(), b->id()});
        std::sort(blocks.begin(), blocks.end());
        blocks.erase(std::unique(blocks.begin(), blocks.end()), blocks.end());
        double fillin = nfree > 0 ? (double)blocks.size() * d * d / ((nfree * d) * (nfree * d)) : 0.0;
        s << "nodes = " << spg_graph_num_vertices(_g) - 1 << "; edges = " << spg_graph_num_edges(_g) << "; fillin = " << fillin * 100 << "%";
    }
    void setEstimate(int vertexid, const IsometryXd &est) override {
        drop_views();
        check(spg_graph_set_estimate(_g, vertexid, est.vector().data()), "setEstimate");
    }

    // ---- beyond the reference interface -----------------------------------------------------------------
    struct EdgeRecord {
        int kind;                    // SPG_EDGE_BINARY | SPG_EDGE_GLC | SPG_EDGE_MULTI
        std::vector<int> vertices;   // ids
        std::vector<double> data;    // record as in spg_batch.edge_data
    };
    std::vector<EdgeRecord> edgeRecords() {
        int ne = spg_graph_num_edges(_g);
        std::vector<int32_t> kind(ne + 1), voff(ne + 1), vids((size_t)spg_graph_edge_vert_size(_g) + 1);
        std::vector<int64_t> doff(ne + 1);
        std::vector<double> data((size_t)spg_graph_edge_data_size(_g) + 1);
        check(spg_graph_get_edges(_g, kind.data(), voff.data(), vids.data(), doff.data(), data.data()), "edges");
        std::vector<EdgeRecord> out(ne);
        for (int e = 0; e < ne; e++) {
            out[e].kind = kind[e];
            out[e].vertices.assign(vids.begin() + voff[e], vids.begin() + voff[e + 1]);
            out[e].data.assign(data.begin() + doff[e], data.begin() + doff[e + 1]);
        }
        return out;
    }
    // sum over blankets of LogdetFunction::value (src/logdet_function.cpp:119-133) of the last marginalize()
    // (GLC graphs: 0 unless setGlcBlanketKld(true) was called before marginalize())
    double lastKullbackLeiblerSum() const { return _stats.kld_sum; }
    // Per-blanket KLD of GLC removals (SPG_FLAG_GLC_KLD, include/spg.h): off by default, as in the reference, whose GLC
    // provider has no LogdetFunction. No effect on an NFR graph. Not a member of the reference's SparsityOptions.
    void setGlcBlanketKld(bool on) { _glc_kld = on; }
    bool glcBlanketKld() const { return _glc_kld; }
    // NFR blankets whose pattern has no closed form (Subgraph / Dense with more than k - 1 edges) by factor descent instead
    // of the interior point (SPG_FLAG_NFR_FACTOR_DESCENT, include/spg.h): off by default; no effect on a GLC graph
    void setFactorDescent(bool on) { _factor_descent = on; }
    bool factorDescent() const { return _factor_descent; }
    const spg_marg_stats &lastStats() const { return _stats; }
    spg_graph *handle() { return _g; }
    spg_ctx *context() { return _ctx->h; }

private:
    GraphWrapperHIP(std::shared_ptr<Ctx> ctx, spg_graph *g, bool glc) : _ctx(std::move(ctx)), _g(g), _glc(glc) {}
    void check(int rc, const char *what) const {
        if (rc < 0) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) + "): " + ((_ctx && _ctx->h) ? spg_last_error(_ctx->h) : ""));
    }
    static std::vector<MatrixXd> split_blocks(const std::vector<double> &buf, int64_t n, int w) {
        std::vector<MatrixXd> out;
        for (int64_t i = 0; i < n; i++) {
            MatrixXd m(w, w);
            std::copy(buf.begin() + i * w * w, buf.begin() + (i + 1) * w * w, m.data());
            out.push_back(std::move(m));
        }
        return out;
    }
    void snapshot(std::vector<int32_t> &ids, std::vector<double> &poses) const {
        int n = spg_graph_num_vertices(_g), ps = spg_graph_pose_dim(_g) == 3 ? 3 : 7;
        ids.resize(n);
        poses.resize((size_t)n * ps);
        check(spg_graph_get_vertices(_g, ids.data(), poses.data()), "vertices");
    }
    void restore(const std::vector<int32_t> &ids, const std::vector<double> &poses) {
        int ps = spg_graph_pose_dim(_g) == 3 ? 3 : 7;
        drop_views();
        for (size_t i = 0; i < ids.size(); i++) check(spg_graph_set_estimate(_g, ids[i], poses.data() + i * ps), "setEstimate");
    }
    void drop_views() const {
        for (Vertex *v : _vviews) delete v;
        for (EdgeView *e : _eviews) delete e;
        _vviews.clear();
        _eviews.clear();
        _views_ok = false;
    }
    void build_views() const {
        if (_views_ok) return;
        drop_views();
        const int d = spg_graph_pose_dim(_g), ps = d == 3 ? 3 : 7;
        std::vector<int32_t> ids;
        std::vector<double> poses;
        snapshot(ids, poses);
        for (size_t i = 0; i < ids.size(); i++) {
            VertexView *v = new VertexView;
            v->_id = ids[i];
            v->_est = IsometryXd(std::vector<double>(poses.begin() + i * ps, poses.begin() + (i + 1) * ps));
            _vviews.push_back(v);
        }
        auto find = [&](int id) -> VertexView * {
            auto it = std::lower_bound(_vviews.begin(), _vviews.end(), id, [](const Vertex *v, int i) { return v->id() < i; });
            return static_cast<VertexView *>(*it);
        };
        std::vector<EdgeRecord> recs = const_cast<GraphWrapperHIP *>(this)->edgeRecords();
        for (EdgeRecord &r : recs) {
            EdgeView *e = new EdgeView;
            e->_kind = r.kind; e->_d = d; e->_rec.swap(r.data);
            for (int id : r.vertices) e->_verts.push_back(find(id));
            _eviews.push_back(e);
            for (size_t i = 0; i < e->_verts.size(); i++) {
                bool dup = false;
                for (size_t j = 0; j < i; j++) dup |= (e->_verts[j] == e->_verts[i]);
                if (!dup) const_cast<VertexView *>(static_cast<const VertexView *>(e->_verts[i]))->_edges.push_back(e);
            }
        }
        _views_ok = true;
    }
    std::shared_ptr<Ctx> _ctx;
    spg_graph *_g = nullptr;
    bool _glc;
    bool _glc_kld = false;
    bool _factor_descent = false;
    spg_marg_stats _stats{};
    spg_optimize_stats _last_opt{};
    mutable std::vector<Vertex *> _vviews;     // id-sorted
    mutable std::vector<EdgeView *> _eviews;   // insertion order of the live edges
    mutable bool _views_ok = false;
};

// ---- computeSubstituteEdge (src/compute_substitute_edge.h:13-16, .cpp:13-96) ---------------------------------
// gw is the FULL source graph; on return the marginalised endpoint of (from, to) is replaced by the nearest
// surviving vertex and edgemeas / edgeinfo hold the composed measurement and sym((sum Omega^-1)^-1).
inline void computeSubstituteEdge(GraphWrapperHIP *gw, const std::vector<int> &marginalized, int maxid, int &from, int &to,
                                  IsometryXd &edgemeas, MatrixXd &edgeinfo) {
    const int d = spg_graph_pose_dim(gw->handle()), ps = d == 3 ? 3 : 7;
    std::vector<int32_t> m(marginalized.begin(), marginalized.end());
    std::vector<double> meas(ps), up((size_t)d * (d + 1) / 2);
    int rc = spg_graph_substitute_edge(gw->handle(), m.data(), (int)m.size(), maxid, &from, &to, meas.data(), up.data());
    if (rc < 0) throw std::runtime_error(std::string("computeSubstituteEdge failed: ") + spg_last_error(gw->context()));
    edgemeas = IsometryXd(meas);
    edgeinfo = MatrixXd(d, d);
    int p = 0;
    for (int i = 0; i < d; i++) for (int j = i; j < d; j++) { edgeinfo(i, j) = edgeinfo(j, i) = up[p]; p++; }
}

}  // namespace spg
