// csrc/spg_host_global.cpp — the entry points of include/spg.h that work on a whole graph at once (global KLD,
// information (dense and block-CSR) and its product, covariance and its blocks, optimize / chi2, the robust kernel and the per-edge chi2, the symbolic plan): the graph is staged on the host as one
// DenseGraphIn and handed to the device drivers of spg_dense.hip / spg_sparse.inc. Nothing here touches the scheduler.
#include "spg_graph_impl.h"
#include "spg_sparse_plan.hpp"
#include "spg_bsr_pattern.hpp"

// ================================================================================= global KLD (a18)
namespace {
struct DenseStage {
    std::vector<int32_t> pos, rowptr, inc, ev;
    std::vector<spg_edge_ref> er;
    spg::DenseGraphIn in;
};

// Live vertex indices in ascending id order.
std::vector<int32_t> live_vertices_by_id(const spg_graph *g) {
    std::vector<int32_t> v;
    for (size_t i = 0; i < g->vid.size(); i++) if (g->valive[i]) v.push_back((int32_t)i);
    std::sort(v.begin(), v.end(), [&](int32_t a, int32_t b) { return g->vid[a] < g->vid[b]; });
    return v;
}

// st.pos must be filled (size = number of vertex slots, -1 = not a variable).
void build_dense_stage(spg_graph *g, DenseStage &st) {
    canonicalize_edge_order(g);
    const int nv = (int)g->vid.size();
    std::vector<int32_t> remap(g->edges.size(), -1);
    for (size_t e = 0; e < g->edges.size(); e++) {
        const GEdge &ge = g->edges[e];
        if (!ge.alive) continue;
        remap[e] = (int32_t)st.er.size();
        st.er.push_back({ge.off, ge.len, ge.kind, (int32_t)st.ev.size(), ge.nv});
        for (int i = 0; i < ge.nv; i++) st.ev.push_back(edge_verts(g, ge)[i]);
    }
    st.rowptr.assign((size_t)nv + 1, 0);
    for (int v = 0; v < nv; v++) {
        if (g->valive[v]) {
            std::vector<int32_t> es;
            for (int32_t e : g->vr[v].adj) if (remap[e] >= 0) es.push_back(remap[e]);
            std::sort(es.begin(), es.end());
            es.erase(std::unique(es.begin(), es.end()), es.end());
            st.inc.insert(st.inc.end(), es.begin(), es.end());
        }
        st.rowptr[v + 1] = (int32_t)st.inc.size();
    }
    st.in.D = g->d; st.in.nv = nv; st.in.ne = (int)st.er.size();
    st.in.pos = st.pos.data(); st.in.vpo = g->vpose.data(); st.in.rowptr = st.rowptr.data(); st.in.inc = st.inc.data();
    st.in.er = st.er.data(); st.in.ev = st.ev.data(); st.in.n_ev = (int64_t)st.ev.size(); st.in.dev_arena = g->dev;
}

int resolve_fixed(const spg_graph *g, const std::vector<int32_t> &order, int32_t fixed_id) {
    if (order.empty()) return -1;
    if (fixed_id < 0) return order[0];   // the reference skips its first (smallest-id) vertex
    auto it = g->vidx.find(fixed_id);
    if (it == g->vidx.end() || !g->valive[it->second]) return -1;
    return it->second;
}

// The live vertices outside `fixed` become the variables, in ascending id order: position = scalar offset (step = d)
// or block number (step = 1).
void stage_free_vertices(spg_graph *g, const std::vector<int32_t> &order, const std::vector<int32_t> &fixed, int step, DenseStage &st) {
    std::vector<uint8_t> is_fixed(g->vid.size(), 0);
    for (int32_t v : fixed) is_fixed[v] = 1;
    st.pos.assign(g->vid.size(), -1);
    int p = 0;
    for (int32_t v : order) if (!is_fixed[v]) { st.pos[v] = p; p += step; }
    build_dense_stage(g, st);
}

// Prologue of a call on one graph: the device holds the graph and is idle, the graph is staged, the error text is clear.
int stage_global(spg_graph *g, const std::vector<int32_t> &order, const std::vector<int32_t> &fixed, int step, DenseStage &st) {
    if (int rc = sync_device(g)) return rc;
    if (int rc = g->ctx->be.synchronize(g->ctx->be.user)) return rc;
    stage_free_vertices(g, order, fixed, step, st);
    g->ctx->err[0] = 0;
    return 0;
}

using DenseMatrixFn = int (*)(void *, const spg::DenseGraphIn &, int, double *, char *, size_t);
// spg_graph_information / spg_graph_covariance: n x n over every live vertex but the fixed one; limit > 0 bounds n
int64_t dense_matrix(spg_graph *g, int32_t fixed_id, double *out, int64_t cap, DenseMatrixFn fn, int64_t limit, const char *what) {
    if (!g || g->active) return SPG_EINVAL;
    std::vector<int32_t> order = live_vertices_by_id(g);
    int fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return set_err(g->ctx, SPG_EINVAL, "%s: the fixed vertex is not in the graph", what);
    const int64_t n = (int64_t)g->d * ((int64_t)order.size() - 1);
    if (!out || cap < n * n) return n;
    if (!g->ctx->is_hip) return set_err(g->ctx, SPG_ESTATE, "%s needs the HIP backend", what);
    if (limit > 0 && n > limit) return set_err(g->ctx, SPG_ECAPACITY, "%s: dense formulation limited to 46k variables", what);
    DenseStage st;
    if (int rc = stage_global(g, order, {fixed}, g->d, st)) return rc;
    int rc = fn(spg::hip_backend_stream(&g->ctx->be), st.in, (int)n, out, g->ctx->err, sizeof g->ctx->err);
    return rc ? rc : n;
}
}  // namespace

extern "C" int64_t spg_graph_information(spg_graph *g, int32_t fixed_id, double *out, int64_t cap) {
    return dense_matrix(g, fixed_id, out, cap, spg::hip_dense_information, 0, "spg_graph_information");
}

// ================================================================================= block-CSR information, H X
namespace {
// What the two calls share: the fixed vertex resolved, the free vertices staged with pos = D * block row (host work
// only unless `device`: then the device holds the graph and is idle) and the pattern of that numbering.
int bsr_stage(spg_graph *g, int32_t fixed_id, bool device, const char *what, std::vector<int32_t> &order, int &fixed, DenseStage &st,
              spg::bsr::Pattern &P) {
    order = live_vertices_by_id(g);
    fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return set_err(g->ctx, SPG_EINVAL, "%s: the fixed vertex is not in the graph", what);
    if (device) {
        if (!g->ctx->is_hip) return set_err(g->ctx, SPG_ESTATE, "%s needs the HIP backend", what);
        if (int rc = stage_global(g, order, {fixed}, g->d, st)) return rc;
    } else {
        stage_free_vertices(g, order, {fixed}, g->d, st);
    }
    spg::bsr::build_pattern(st.in.nv, st.in.pos, g->d, st.in.ne, st.in.er, st.in.ev, P);
    return 0;
}
}  // namespace

extern "C" int64_t spg_graph_sparse_information(spg_graph *g, int32_t fixed_id, int64_t *row_ptr, int32_t *col_idx, double *blocks,
                                                int64_t cap_blocks, int32_t *ids) {
    if (!g || g->active || cap_blocks < 0) return SPG_EINVAL;
    std::vector<int32_t> order;
    int fixed = -1;
    DenseStage st;
    spg::bsr::Pattern P;
    const bool values = blocks && row_ptr && col_idx;
    if (int rc = bsr_stage(g, fixed_id, false, "spg_graph_sparse_information", order, fixed, st, P)) return rc;
    const int64_t nnzb = P.nnzb();
    if (!row_ptr || !col_idx || cap_blocks < nnzb) return nnzb;
    if (values) {
        // the device copy of the graph may move when it is brought up to date: stage again once it is
        DenseStage sd;
        if (int rc = bsr_stage(g, fixed_id, true, "spg_graph_sparse_information", order, fixed, sd, P)) return rc;
        if (int rc = spg::hip_bsr_information(spg::hip_backend_stream(&g->ctx->be), sd.in, P, blocks, g->ctx->err, sizeof g->ctx->err)) return rc;
    }
    std::copy(P.row_ptr.begin(), P.row_ptr.end(), row_ptr);
    std::copy(P.col.begin(), P.col.end(), col_idx);
    if (ids) {
        int32_t *o = ids;
        for (int32_t v : order) if (v != fixed) *o++ = g->vid[v];
    }
    return nnzb;
}

extern "C" int spg_graph_information_apply(spg_graph *g, int32_t fixed_id, const double *X, int nrhs, double *Y) {
    if (!g || g->active || !X || !Y || nrhs <= 0) return SPG_EINVAL;
    std::vector<int32_t> order;
    int fixed = -1;
    DenseStage st;
    spg::bsr::Pattern P;
    if (int rc = bsr_stage(g, fixed_id, true, "spg_graph_information_apply", order, fixed, st, P)) return rc;
    return spg::hip_bsr_apply(spg::hip_backend_stream(&g->ctx->be), st.in, P, X, nrhs, Y, g->ctx->err, sizeof g->ctx->err);
}

extern "C" int spg_debug_bsr_bench(spg_graph *g, int32_t fixed_id, int reps, double *out) {
    if (!g || g->active || !out || reps <= 0) return SPG_EINVAL;
    std::vector<int32_t> order;
    int fixed = -1;
    DenseStage st;
    spg::bsr::Pattern P;
    if (int rc = bsr_stage(g, fixed_id, true, "spg_debug_bsr_bench", order, fixed, st, P)) return rc;
    return spg::hip_bsr_bench(spg::hip_backend_stream(&g->ctx->be), st.in, P, reps, out, g->ctx->err, sizeof g->ctx->err);
}

extern "C" int64_t spg_graph_covariance(spg_graph *g, int32_t fixed_id, double *out, int64_t cap) {
    return dense_matrix(g, fixed_id, out, cap, spg::hip_dense_covariance, 46000, "spg_graph_covariance");
}

extern "C" int spg_graph_kullback_leibler(spg_graph *base, spg_graph *other, int32_t fixed_id, spg_kld_terms *out) {
    if (!base || !other || !out || base->active || other->active) return SPG_EINVAL;
    spg_ctx *ctx = base->ctx;
    if (base->d != other->d) return set_err(ctx, SPG_EINVAL, "spg_graph_kullback_leibler: pose dimensions differ");
    if (!ctx->is_hip || !other->ctx->is_hip) return set_err(ctx, SPG_ESTATE, "spg_graph_kullback_leibler needs the HIP backend");
    if (spg::hip_backend_device(&ctx->be) != spg::hip_backend_device(&other->ctx->be))
        return set_err(ctx, SPG_EINVAL, "spg_graph_kullback_leibler: both graphs must live on the same device");
    const int d = base->d;
    std::vector<int32_t> ob = live_vertices_by_id(base), oo = live_vertices_by_id(other);
    int fb = resolve_fixed(base, ob, fixed_id);
    if (fb < 0) return set_err(ctx, SPG_EINVAL, "spg_graph_kullback_leibler: the fixed vertex is not in the baseline");
    const int32_t fid = base->vid[fb];
    int fo = resolve_fixed(other, oo, fid);
    if (fo < 0) return set_err(ctx, SPG_EINVAL, "spg_graph_kullback_leibler: the fixed vertex is not in the sparsified graph");
    // computeIndices (src/graph_wrapper_g2o.cpp:472-499): merge of the two id-sorted vertex lists
    std::vector<int32_t> kept_b, kept_o, marg_b;
    {
        size_t j = 0;
        for (int32_t v : ob) {
            if (v == fb) continue;
            while (j < oo.size() && (oo[j] == fo || other->vid[oo[j]] < base->vid[v])) {
                if (oo[j] != fo) return set_err(ctx, SPG_EINVAL, "spg_graph_kullback_leibler: the sparsified graph holds a vertex the baseline lacks");
                j++;
            }
            if (j < oo.size() && other->vid[oo[j]] == base->vid[v]) { kept_b.push_back(v); kept_o.push_back(oo[j]); j++; }
            else marg_b.push_back(v);
        }
        for (; j < oo.size(); j++)
            if (oo[j] != fo) return set_err(ctx, SPG_EINVAL, "spg_graph_kullback_leibler: the sparsified graph holds a vertex the baseline lacks");
    }
    if (kept_b.empty()) return set_err(ctx, SPG_EINVAL, "spg_graph_kullback_leibler: no common free vertex");
    const int64_t n_marg = (int64_t)d * marg_b.size(), n_keep = (int64_t)d * kept_b.size();
    const int64_t Nm = (n_marg + 63) / 64 * 64, Ng = (n_keep + 63) / 64 * 64;
    // (PCG yields no log-determinant: the KLD treats it as AUTO)
    const int solver = ctx->linear_solver == SPG_SOLVER_PCG ? (int)SPG_SOLVER_AUTO : ctx->linear_solver;
    const bool sparse = solver == SPG_SOLVER_SPARSE || (solver == SPG_SOLVER_AUTO && Nm + Ng > 46000);
    if (!sparse && Nm + Ng > 46000) return set_err(ctx, SPG_ECAPACITY, "spg_graph_kullback_leibler: dense formulation limited to 46k variables (16 GB)");
    if (int rc = sync_device(base)) return rc;
    if (int rc = sync_device(other)) return rc;
    if (int rc = ctx->be.synchronize(ctx->be.user)) return rc;
    if (other->ctx != ctx) if (int rc = other->ctx->be.synchronize(other->ctx->be.user)) return rc;
    spg_kld_terms t{};   // the drivers add to the counters and seconds of the struct they are handed
    t.n_marginalized = n_marg;
    t.solver = sparse ? SPG_SOLVER_SPARSE : SPG_SOLVER_DENSE;
    DenseStage sb, so;
    sb.pos.assign(base->vid.size(), -1);
    so.pos.assign(other->vid.size(), -1);
    std::vector<int64_t> kvb, kvo;
    for (size_t i = 0; i < kept_b.size(); i++) { kvb.push_back(base->vpose[kept_b[i]]); kvo.push_back(other->vpose[kept_o[i]]); }
    void *stream = spg::hip_backend_stream(&ctx->be);
    int rc;
    if (sparse) {
        // block-sparse multifrontal path: positions only number the blocks, the elimination order is the plan's
        std::vector<uint8_t> is_marg(base->vid.size(), 0);
        int p = 0;
        for (int32_t v : ob) if (v != fb) sb.pos[v] = p++;
        for (int32_t v : marg_b) is_marg[v] = 1;
        for (size_t i = 0; i < kept_b.size(); i++) so.pos[kept_o[i]] = (int32_t)i;
        build_dense_stage(base, sb);
        build_dense_stage(other, so);
        ctx->err[0] = 0;
        rc = spg::hip_sparse_kld(stream, sb.in, so.in, is_marg.data(), kept_b.data(), kept_o.data(), (int)kept_b.size(), kvb.data(), kvo.data(), t,
                                 ctx->err, sizeof ctx->err);
    } else {
        int p = 0;
        for (int32_t v : marg_b) { sb.pos[v] = p; p += d; }
        for (size_t i = 0; i < kept_b.size(); i++) { sb.pos[kept_b[i]] = (int32_t)(Nm + d * i); so.pos[kept_o[i]] = (int32_t)(d * i); }
        build_dense_stage(base, sb);
        build_dense_stage(other, so);
        ctx->err[0] = 0;
        rc = spg::hip_dense_kld(stream, sb.in, so.in, (int)n_marg, (int)n_keep, kvb.data(), kvo.data(), t, ctx->err, sizeof ctx->err);
    }
    if (rc) return rc;
    *out = t;
    return 0;
}

// ================================================================================= covariance blocks (sparse factor)
namespace {
int live_index(const spg_graph *g, int32_t id) {
    auto it = g->vidx.find(id);
    return (it == g->vidx.end() || !g->valive[it->second]) ? -1 : it->second;
}
bool share_live_edge(const spg_graph *g, int32_t a, int32_t b) {
    for (int32_t e : g->vr[a].adj) {
        const GEdge &ge = g->edges[e];
        if (!ge.alive) continue;
        const int32_t *vs = edge_verts(g, ge);
        for (int i = 0; i < ge.nv; i++) if (vs[i] == b) return true;
    }
    return false;
}
// What cov_blocks and cov_solve share. Each list of vertex indices names the fixed vertex as -1 from here on. Returns 1 when
// the graph holds nothing but the fixed vertex (every block is zero: out is filled), 0 when the graph is staged
// (every live vertex but the fixed one is a block, numbered by ascending id), < 0 on an error.
int cov_stage(spg_graph *g, int fixed, const std::vector<int32_t> &order, std::initializer_list<std::vector<int32_t> *> lists, int64_t need,
              double *out, const char *what, DenseStage &st) {
    if (!g->ctx->is_hip) return set_err(g->ctx, SPG_ESTATE, "%s needs the HIP backend", what);
    for (std::vector<int32_t> *l : lists) for (int32_t &v : *l) if (v == fixed) v = -1;
    if (need == 0 || order.size() < 2) {
        std::fill(out, out + need, 0.0);
        return 1;
    }
    return stage_global(g, order, {fixed}, 1, st);
}
// K vertex indices per request (-1 = the fixed vertex) -> (K D)^2 doubles per request
int64_t cov_blocks(spg_graph *g, int fixed, const std::vector<int32_t> &order, int K, std::vector<int32_t> &req, double *out,
                   spg_cov_stats *stats, const char *what) {
    const int64_t n = (int64_t)req.size() / K, W = (int64_t)K * g->d, need = n * W * W;
    DenseStage st;
    spg_cov_stats cs{};
    const int staged = cov_stage(g, fixed, order, {&req}, need, out, what, st);
    if (staged < 0) return staged;
    if (staged == 0)
        if (int rc = spg::hip_sparse_cov_blocks(spg::hip_backend_stream(&g->ctx->be), st.in, K, req.data(), (int)n, out, cs, g->ctx->err, sizeof g->ctx->err)) return rc;
    if (stats) *stats = cs;
    return need;
}
}  // namespace

extern "C" int64_t spg_graph_marginal_covariances(spg_graph *g, int32_t fixed_id, const int32_t *ids, int n, double *out, int64_t cap,
                                                  spg_cov_stats *stats) {
    if (!g || g->active || (ids && n < 0)) return SPG_EINVAL;
    std::vector<int32_t> order = live_vertices_by_id(g);
    const int fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return set_err(g->ctx, SPG_EINVAL, "spg_graph_marginal_covariances: the fixed vertex is not in the graph");
    std::vector<int32_t> req;
    if (!ids) req = order;
    else {
        req.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            req[i] = live_index(g, ids[i]);
            if (req[i] < 0) {
                snprintf(g->ctx->err, sizeof g->ctx->err, "spg_graph_marginal_covariances: vertex %d is not in the graph", (int)ids[i]);
                return SPG_EINVAL;
            }
        }
    }
    const int64_t need = (int64_t)req.size() * g->d * g->d;
    if (!out || cap < need) return need;
    return cov_blocks(g, fixed, order, 1, req, out, stats, "spg_graph_marginal_covariances");
}

extern "C" int64_t spg_graph_joint_covariances(spg_graph *g, int32_t fixed_id, const int32_t *pairs, int n, double *out, int64_t cap,
                                               spg_cov_stats *stats) {
    if (!g || g->active || n < 0 || (n > 0 && !pairs)) return SPG_EINVAL;
    std::vector<int32_t> order = live_vertices_by_id(g);
    const int fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return set_err(g->ctx, SPG_EINVAL, "spg_graph_joint_covariances: the fixed vertex is not in the graph");
    std::vector<int32_t> req((size_t)2 * n);
    for (int i = 0; i < n; i++) {
        const int32_t a = pairs[2 * i], b = pairs[2 * i + 1];
        const int va = live_index(g, a), vb = live_index(g, b);
        const char *why = (va < 0 || vb < 0) ? "a vertex is not in the graph" : (a == b) ? "the two vertices are the same"
                          : !share_live_edge(g, va, vb) ? "the vertices share no live edge" : nullptr;
        if (why) {
            snprintf(g->ctx->err, sizeof g->ctx->err, "spg_graph_joint_covariances: pair %d (%d, %d): %s", i, (int)a, (int)b, why);
            return SPG_EINVAL;
        }
        req[2 * i] = va;
        req[2 * i + 1] = vb;
    }
    const int64_t W = 2 * g->d, need = (int64_t)n * W * W;
    if (!out || cap < need) return need;
    return cov_blocks(g, fixed, order, 2, req, out, stats, "spg_graph_joint_covariances");
}

extern "C" int spg_graph_marginal_kld(spg_graph *base, spg_graph *other, int32_t fixed_id, int32_t *ids, double *kld, int cap,
                                      spg_cov_stats *stats) {
    if (!base || !other || base->active || other->active) return SPG_EINVAL;
    spg_ctx *ctx = base->ctx;
    if (base->d != other->d) return set_err(ctx, SPG_EINVAL, "spg_graph_marginal_kld: pose dimensions differ");
    std::vector<int32_t> ob = live_vertices_by_id(base), oo = live_vertices_by_id(other);
    const int fb = resolve_fixed(base, ob, fixed_id);
    if (fb < 0) return set_err(ctx, SPG_EINVAL, "spg_graph_marginal_kld: the fixed vertex is not in the baseline");
    const int fo = resolve_fixed(other, oo, base->vid[fb]);
    if (fo < 0) return set_err(ctx, SPG_EINVAL, "spg_graph_marginal_kld: the fixed vertex is not in the sparsified graph");
    std::vector<int32_t> vb, vo, out_ids;
    for (int32_t v : oo) {
        if (v == fo) continue;
        const int u = live_index(base, other->vid[v]);
        if (u < 0) {
            snprintf(ctx->err, sizeof ctx->err, "spg_graph_marginal_kld: the sparsified graph holds vertex %d, which the baseline lacks", (int)other->vid[v]);
            return SPG_EINVAL;
        }
        vb.push_back(u);
        vo.push_back(v);
        out_ids.push_back(other->vid[v]);
    }
    const int nk = (int)vo.size();
    if (!ids || !kld || cap < nk) return nk;
    if (!ctx->is_hip || !other->ctx->is_hip) return set_err(ctx, SPG_ESTATE, "spg_graph_marginal_kld needs the HIP backend");
    if (spg::hip_backend_device(&ctx->be) != spg::hip_backend_device(&other->ctx->be))
        return set_err(ctx, SPG_EINVAL, "spg_graph_marginal_kld: both graphs must live on the same device");
    spg_cov_stats cs{};
    if (nk > 0) {
        if (int rc = sync_device(base)) return rc;
        if (int rc = sync_device(other)) return rc;
        if (int rc = ctx->be.synchronize(ctx->be.user)) return rc;
        if (other->ctx != ctx) if (int rc = other->ctx->be.synchronize(other->ctx->be.user)) return rc;
        DenseStage sb, so;
        stage_free_vertices(base, ob, {fb}, 1, sb);
        stage_free_vertices(other, oo, {fo}, 1, so);
        std::vector<int64_t> kvb, kvo;
        for (int i = 0; i < nk; i++) { kvb.push_back(base->vpose[vb[i]]); kvo.push_back(other->vpose[vo[i]]); }
        ctx->err[0] = 0;
        int rc = spg::hip_sparse_marginal_kld(spg::hip_backend_stream(&ctx->be), sb.in, so.in, vb.data(), vo.data(), nk, kvb.data(), kvo.data(),
                                              kld, cs, ctx->err, sizeof ctx->err);
        if (rc) return rc;
    }
    std::copy(out_ids.begin(), out_ids.end(), ids);
    if (stats) *stats = cs;
    return nk;
}

// ================================================================================= covariance of arbitrary pairs / sets
namespace {
// D x D sub-blocks Sigma(va[i], vb[i]) (vertex indices) at out + dst[i], row stride ld
int64_t cov_solve(spg_graph *g, int fixed, const std::vector<int32_t> &order, std::vector<int32_t> &va, std::vector<int32_t> &vb,
                  const std::vector<int64_t> &dst, int32_t ld, int64_t need, double *out, spg_cov_solve_stats *stats, const char *what) {
    DenseStage st;
    spg_cov_solve_stats cs{};
    const int staged = cov_stage(g, fixed, order, {&va, &vb}, need, out, what, st);
    if (staged < 0) return staged;
    if (staged == 0)
        if (int rc = spg::hip_sparse_cov_solve(spg::hip_backend_stream(&g->ctx->be), st.in, va.data(), vb.data(), dst.data(), ld, (int64_t)va.size(), need, out,
                                               cs, g->ctx->err, sizeof g->ctx->err)) return rc;
    if (stats) *stats = cs;
    return need;
}
}  // namespace

extern "C" int64_t spg_graph_pair_covariances(spg_graph *g, int32_t fixed_id, const int32_t *pairs, int n, double *out, int64_t cap,
                                              spg_cov_solve_stats *stats) {
    if (!g || g->active || n < 0 || (n > 0 && !pairs)) return SPG_EINVAL;
    std::vector<int32_t> order = live_vertices_by_id(g);
    const int fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return set_err(g->ctx, SPG_EINVAL, "spg_graph_pair_covariances: the fixed vertex is not in the graph");
    const int D = g->d;
    const int64_t W = 2 * D, need = (int64_t)n * W * W;
    std::vector<int32_t> va, vb;
    std::vector<int64_t> dst;
    for (int i = 0; i < n; i++) {
        const int32_t a = pairs[2 * i], b = pairs[2 * i + 1];
        const int ia = live_index(g, a), ib = live_index(g, b);
        const char *why = (ia < 0 || ib < 0) ? "a vertex is not in the graph" : (a == b) ? "the two vertices are the same" : nullptr;
        if (why) {
            snprintf(g->ctx->err, sizeof g->ctx->err, "spg_graph_pair_covariances: pair %d (%d, %d): %s", i, (int)a, (int)b, why);
            return SPG_EINVAL;
        }
        if (!out || cap < need) continue;
        const int32_t v[2] = {ia, ib};
        for (int ka = 0; ka < 2; ka++)
            for (int kb = 0; kb < 2; kb++) { va.push_back(v[ka]); vb.push_back(v[kb]); dst.push_back(i * W * W + ka * D * W + kb * D); }
    }
    if (!out || cap < need) return need;
    return cov_solve(g, fixed, order, va, vb, dst, (int32_t)W, need, out, stats, "spg_graph_pair_covariances");
}

extern "C" int64_t spg_graph_joint_marginal_covariance(spg_graph *g, int32_t fixed_id, const int32_t *ids, int n, double *out, int64_t cap,
                                                       spg_cov_solve_stats *stats) {
    if (!g || g->active || n < 0 || (n > 0 && !ids)) return SPG_EINVAL;
    std::vector<int32_t> order = live_vertices_by_id(g);
    const int fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return set_err(g->ctx, SPG_EINVAL, "spg_graph_joint_marginal_covariance: the fixed vertex is not in the graph");
    const int D = g->d;
    const int64_t W = (int64_t)n * D, need = W * W;
    if (W > 46000)
        return set_err(g->ctx, SPG_ECAPACITY, "spg_graph_joint_marginal_covariance: limited to 46k variables, the bound of spg_graph_covariance");
    std::vector<int32_t> idx((size_t)n);
    {
        std::unordered_set<int32_t> seen;
        for (int i = 0; i < n; i++) {
            idx[i] = live_index(g, ids[i]);
            const char *why = idx[i] < 0 ? "is not in the graph" : !seen.insert(ids[i]).second ? "is listed twice" : nullptr;
            if (why) {
                snprintf(g->ctx->err, sizeof g->ctx->err, "spg_graph_joint_marginal_covariance: vertex %d %s", (int)ids[i], why);
                return SPG_EINVAL;
            }
        }
    }
    if (!out || cap < need) return need;
    std::vector<int32_t> va, vb;
    std::vector<int64_t> dst;
    va.reserve((size_t)n * n); vb.reserve((size_t)n * n); dst.reserve((size_t)n * n);
    for (int a = 0; a < n; a++)
        for (int b = 0; b < n; b++) { va.push_back(idx[a]); vb.push_back(idx[b]); dst.push_back((int64_t)a * D * W + (int64_t)b * D); }
    return cov_solve(g, fixed, order, va, vb, dst, (int32_t)W, need, out, stats, "spg_graph_joint_marginal_covariance");
}

// ================================================================================= relative covariances, candidate scores
namespace {
// Candidate i of relative_call / select_call, ij[2i] -> ij[2i+1] with record i of `records` (may be nullptr): its vertex
// indices, or SPG_EINVAL with the pair named.
int check_pair(spg_graph *g, const char *what, int i, const int32_t *ij, const double *records, int &ia, int &ib) {
    const int32_t a = ij[2 * i], b = ij[2 * i + 1];
    ia = live_index(g, a);
    ib = live_index(g, b);
    const char *why = (ia < 0 || ib < 0) ? "a vertex is not in the graph" : (a == b) ? "the two vertices are the same" : nullptr;
    if (!why && records)
        for (int k = 0; k < g->ps; k++) if (!std::isfinite(records[(size_t)i * g->rec + k])) why = "the measurement is not finite";
    if (!why) return 0;
    snprintf(g->ctx->err, sizeof g->ctx->err, "%s: pair %d (%d, %d): %s", what, i, (int)a, (int)b, why);
    return SPG_EINVAL;
}
// What spg_graph_relative_covariances and spg_graph_score_candidates share. n hypothetical binary edges ij[2i] -> ij[2i+1]
// (records == nullptr: measured at the current relative pose) are checked; when `compute`, one 2D x 2D block per distinct
// ordered pair is solved for and stays on the device, where sp_relative_kernel turns it into the results. Returns `ret`.
int64_t relative_call(spg_graph *g, int32_t fixed_id, const int32_t *ij, int n, const double *records, bool compute, int64_t ret, double *rel,
                      double *cov, double *d2, double *gain, double *chi2, int32_t *status, spg_cov_solve_stats *stats, const char *what) {
    if (!g || n < 0 || (n > 0 && !ij)) return SPG_EINVAL;
    if (g->active) return set_err(g->ctx, SPG_EINVAL, "%s: a stepwise marginalisation is active", what);
    std::vector<int32_t> order = live_vertices_by_id(g);
    const int fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return set_err(g->ctx, SPG_EINVAL, "%s: the fixed vertex is not in the graph", what);
    const int D = g->d;
    const int64_t W = 2 * D;
    std::vector<int32_t> va, vb, ca, cb, slot;
    std::vector<int64_t> dst;
    std::unordered_map<uint64_t, int32_t> slot_of;
    for (int i = 0; i < n; i++) {
        int ia, ib;
        if (int rc = check_pair(g, what, i, ij, records, ia, ib)) return rc;
        if (!compute) continue;
        auto it = slot_of.emplace(((uint64_t)(uint32_t)ia << 32) | (uint32_t)ib, (int32_t)slot_of.size());
        if (it.second) {
            const int32_t v[2] = {ia, ib};
            const int64_t u = it.first->second;
            for (int ka = 0; ka < 2; ka++)
                for (int kb = 0; kb < 2; kb++) { va.push_back(v[ka]); vb.push_back(v[kb]); dst.push_back(u * W * W + ka * D * W + kb * D); }
        }
        ca.push_back(ia); cb.push_back(ib); slot.push_back(it.first->second);
    }
    if (!compute) return ret;
    DenseStage st;
    spg_cov_solve_stats cs{};
    const int64_t blocks_len = (int64_t)slot_of.size() * W * W;
    const int staged = cov_stage(g, fixed, order, {&va, &vb}, blocks_len, nullptr, what, st);
    if (staged < 0) return staged;
    if (staged == 0)
        if (int rc = spg::hip_sparse_relative(spg::hip_backend_stream(&g->ctx->be), st.in, va.data(), vb.data(), dst.data(), (int32_t)W, (int64_t)va.size(),
                                              blocks_len, ca.data(), cb.data(), slot.data(), n, records, rel, cov, d2, gain, chi2, status, cs, g->ctx->err,
                                              sizeof g->ctx->err)) return rc;
    if (stats) *stats = cs;
    return ret;
}
}  // namespace

extern "C" int64_t spg_graph_relative_covariances(spg_graph *g, int32_t fixed_id, const int32_t *pairs, int n, double *rel, double *cov,
                                                  int64_t cap, spg_cov_solve_stats *stats) {
    const int64_t need = g ? (int64_t)std::max(n, 0) * g->d * g->d : 0;
    return relative_call(g, fixed_id, pairs, n, nullptr, cov && cap >= need, need, rel, cov, nullptr, nullptr, nullptr, nullptr, stats,
                         "spg_graph_relative_covariances");
}

extern "C" int spg_graph_score_candidates(spg_graph *g, int32_t fixed_id, const int32_t *ij, const double *records, int n, double *d2,
                                          double *gain, double *chi2, int32_t *status, int cap, spg_cov_solve_stats *stats) {
    if (n > 0 && !records) return SPG_EINVAL;
    return (int)relative_call(g, fixed_id, ij, n, n > 0 ? records : nullptr, cap >= n, n, nullptr, nullptr, d2, gain, chi2, status, stats,
                              "spg_graph_score_candidates");
}

// ================================================================================= greedy candidate selection
namespace {
// Round-0 state of the lazy greedy calls: one 2D x 2D block per distinct ordered pair of vertex indices, the list
// relative_call builds (sub-block lists of cov_solve_device, row stride 2D), and per candidate the slot of its block.
struct PairBlocks {
    std::vector<int32_t> va, vb, slot;
    std::vector<int64_t> dst;
    std::unordered_map<uint64_t, int32_t> slot_of;
    void add(int32_t ia, int32_t ib, int D) {
        const int64_t W = 2 * D;
        auto it = slot_of.emplace(((uint64_t)(uint32_t)ia << 32) | (uint32_t)ib, (int32_t)slot_of.size());
        if (it.second) {
            const int32_t v[2] = {ia, ib};
            const int64_t u = it.first->second;
            for (int ka = 0; ka < 2; ka++)
                for (int kb = 0; kb < 2; kb++) { va.push_back(v[ka]); vb.push_back(v[kb]); dst.push_back(u * W * W + ka * D * W + kb * D); }
        }
        slot.push_back(it.first->second);
    }
    int64_t len(int D) const { return (int64_t)slot_of.size() * 4 * D * D; }
};
// spg_ctx_greedy_stats after a call that took the joint block
void joint_greedy_stats(spg_ctx *c, int rounds) {
    c->greedy_stats = spg_greedy_stats{};
    c->greedy_stats.method = SPG_GREEDY_JOINT;
    c->greedy_stats.rounds = rounds;
}
// spg_graph_select_candidates: the checks of relative_call, then the endpoint set S (distinct non-fixed endpoints in
// first-appearance order), the sub-block list of its m x m joint covariance as spg_graph_joint_marginal_covariance builds
// it, and per candidate the slots of its endpoints in S (-1 = the fixed vertex).
int select_call(spg_graph *g, int32_t fixed_id, const int32_t *ij, const double *records, int n, int k, double min_gain, double max_d2,
                int32_t *selected, double *cond_gain, int cap, double *final_gain, int32_t *status, spg_select_stats *stats) {
    const char *what = "spg_graph_select_candidates";
    if (!g || n < 0 || (n > 0 && (!ij || !records))) return SPG_EINVAL;
    if (k < 0) return set_err(g->ctx, SPG_EINVAL, "%s: k is negative", what);
    if (g->active) return set_err(g->ctx, SPG_EINVAL, "%s: a stepwise marginalisation is active", what);
    std::vector<int32_t> order = live_vertices_by_id(g);
    const int fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return set_err(g->ctx, SPG_EINVAL, "%s: the fixed vertex is not in the graph", what);
    const int D = g->d;
    std::vector<int32_t> S, ca((size_t)n), cb((size_t)n), sa((size_t)n), sb((size_t)n);
    std::unordered_map<int32_t, int32_t> slot_of;
    for (int i = 0; i < n; i++) {
        int ia, ib;
        if (int rc = check_pair(g, what, i, ij, records, ia, ib)) return rc;
        ca[i] = ia; cb[i] = ib;
        const int32_t v[2] = {ia, ib};
        int32_t sl[2];
        for (int e = 0; e < 2; e++) {
            if (v[e] == fixed) { sl[e] = -1; continue; }
            auto it = slot_of.emplace(v[e], (int32_t)S.size());
            if (it.second) S.push_back(v[e]);
            sl[e] = it.first->second;
        }
        sa[i] = sl[0]; sb[i] = sl[1];
    }
    const int kk = std::min(k, n);
    if (kk == 0) return 0;
    const int64_t m = (int64_t)S.size(), W = m * D, need = W * W;
    const int method = g->ctx->greedy_method;
    if (method == SPG_GREEDY_JOINT && W > 46000) {
        snprintf(g->ctx->err, sizeof g->ctx->err, "%s: %lld distinct endpoints, limited to 46k variables, the bound of spg_graph_joint_marginal_covariance",
                 what, (long long)m);
        return SPG_ECAPACITY;
    }
    if (!selected || !cond_gain || cap < kk) return kk;
    spg_select_stats ss{};
    ss.endpoints = (int32_t)m;
    int nsel = 0;
    if (method == SPG_GREEDY_JOINT || (method == SPG_GREEDY_AUTO && W <= 46000)) {
        std::vector<int32_t> va, vb;
        std::vector<int64_t> dst;
        va.reserve((size_t)(m * m)); vb.reserve((size_t)(m * m)); dst.reserve((size_t)(m * m));
        for (int64_t a = 0; a < m; a++)
            for (int64_t b = 0; b < m; b++) { va.push_back(S[a]); vb.push_back(S[b]); dst.push_back(a * D * W + b * D); }
        DenseStage st;
        const int staged = cov_stage(g, fixed, order, {&va, &vb}, need, nullptr, what, st);
        if (staged < 0) return staged;
        const int rc = spg::hip_sparse_select(spg::hip_backend_stream(&g->ctx->be), st.in, va.data(), vb.data(), dst.data(), (int32_t)W, (int64_t)va.size(), need,
                                              ca.data(), cb.data(), sa.data(), sb.data(), n, records, kk, min_gain, max_d2, selected, cond_gain, final_gain,
                                              status, &nsel, ss, g->ctx->err, sizeof g->ctx->err);
        if (rc == 0) {
            joint_greedy_stats(g->ctx, ss.rounds);
            if (stats) *stats = ss;
            return nsel;
        }
        if (!(method == SPG_GREEDY_AUTO && rc == SPG_ECAPACITY)) return rc;   // AUTO: what JOINT cannot hold goes to LAZY
        ss = spg_select_stats{};
        ss.endpoints = (int32_t)m;
    }
    PairBlocks pb;
    for (int i = 0; i < n; i++) pb.add(ca[i], cb[i], D);
    DenseStage st;
    const int staged = cov_stage(g, fixed, order, {&pb.va, &pb.vb}, pb.len(D), nullptr, what, st);
    if (staged < 0) return staged;
    const spg::GreedyLazyIn lz{pb.slot.data(), S.data(), (int)m, g->ctx->greedy_lookahead, &g->ctx->greedy_stats};
    if (int rc = spg::hip_sparse_select(spg::hip_backend_stream(&g->ctx->be), st.in, pb.va.data(), pb.vb.data(), pb.dst.data(), (int32_t)(2 * D),
                                        (int64_t)pb.va.size(), pb.len(D), ca.data(), cb.data(), sa.data(), sb.data(), n, records, kk, min_gain, max_d2,
                                        selected, cond_gain, final_gain, status, &nsel, ss, g->ctx->err, sizeof g->ctx->err, &lz)) return rc;
    if (stats) *stats = ss;
    return nsel;
}
}  // namespace

extern "C" int spg_graph_select_candidates(spg_graph *g, int32_t fixed_id, const int32_t *ij, const double *records, int n, int k, double min_gain,
                                           double max_d2, int32_t *selected, double *cond_gain, int cap, double *final_gain, int32_t *status,
                                           spg_select_stats *stats) {
    return select_call(g, fixed_id, ij, records, n, k, min_gain, max_d2, selected, cond_gain, cap, final_gain, status, stats);
}

// ================================================================================= joint compatibility of candidates
namespace {
constexpr int kCompatMaxN = 16384;
// set_err with numbers in the text
template <class... A>
int fail(spg_ctx *c, int code, const char *fmt, A... a) {
    snprintf(c->err, sizeof c->err, fmt, a...);
    return code;
}
// spg_graph_compatible_candidates: the checks, the endpoint set and the slots of select_call, the joint block always.
int compat_call(spg_graph *g, int32_t fixed_id, const int32_t *ij, const double *records, int n, int k, double max_d2, double pair_max_d2,
                const double *joint_max_d2, int32_t *compatible, double *joint_d2, int cap, int32_t *clique, int clique_cap, double *d2, int32_t *degree,
                int32_t *status, double *pair_d2, int64_t pair_cap, spg_compat_stats *stats) {
    const char *what = "spg_graph_compatible_candidates";
    if (!g || n < 0 || (n > 0 && (!ij || !records))) return SPG_EINVAL;
    if (k < 0) return set_err(g->ctx, SPG_EINVAL, "%s: k is negative", what);
    if (!(pair_max_d2 > 0.0)) return set_err(g->ctx, SPG_EINVAL, "%s: pair_max_d2 must be positive", what);
    if (clique && clique_cap < n) return set_err(g->ctx, SPG_EINVAL, "%s: clique_cap is below n", what);
    if (pair_d2 && pair_cap < (int64_t)n * n) return set_err(g->ctx, SPG_EINVAL, "%s: pair_cap is below n^2", what);
    if (g->active) return set_err(g->ctx, SPG_EINVAL, "%s: a stepwise marginalisation is active", what);
    std::vector<int32_t> order = live_vertices_by_id(g);
    const int fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return set_err(g->ctx, SPG_EINVAL, "%s: the fixed vertex is not in the graph", what);
    const int D = g->d;
    std::vector<int32_t> S, ca((size_t)n), cb((size_t)n), sa((size_t)n), sb((size_t)n);
    std::unordered_map<int32_t, int32_t> slot_of;
    for (int i = 0; i < n; i++) {
        int ia, ib;
        if (int rc = check_pair(g, what, i, ij, records, ia, ib)) return rc;
        ca[i] = ia; cb[i] = ib;
        const int32_t v[2] = {ia, ib};
        int32_t sl[2];
        for (int e = 0; e < 2; e++) {
            if (v[e] == fixed) { sl[e] = -1; continue; }
            auto it = slot_of.emplace(v[e], (int32_t)S.size());
            if (it.second) S.push_back(v[e]);
            sl[e] = it.first->second;
        }
        sa[i] = sl[0]; sb[i] = sl[1];
    }
    const int kk = std::min(k, n);
    if (kk == 0) return 0;
    const int64_t m = (int64_t)S.size(), W = m * D, need = W * W;
    if (n > kCompatMaxN) return fail(g->ctx, SPG_ECAPACITY, "%s: %d candidates, limited to %d", what, n, kCompatMaxN);
    if (W > 46000) {
        snprintf(g->ctx->err, sizeof g->ctx->err, "%s: %lld distinct endpoints, limited to 46k variables, the bound of spg_graph_joint_marginal_covariance",
                 what, (long long)m);
        return SPG_ECAPACITY;
    }
    if (!compatible || !joint_d2 || cap < kk) return kk;
    std::vector<int32_t> va, vb;
    std::vector<int64_t> dst;
    va.reserve((size_t)(m * m)); vb.reserve((size_t)(m * m)); dst.reserve((size_t)(m * m));
    for (int64_t a = 0; a < m; a++)
        for (int64_t b = 0; b < m; b++) { va.push_back(S[a]); vb.push_back(S[b]); dst.push_back(a * D * W + b * D); }
    DenseStage st;
    const int staged = cov_stage(g, fixed, order, {&va, &vb}, need, nullptr, what, st);
    if (staged < 0) return staged;
    spg_compat_stats cs{};
    cs.endpoints = (int32_t)m;
    int nacc = 0;
    const spg::CompatOut out{compatible, joint_d2, clique, d2, degree, status, pair_d2};
    if (int rc = spg::hip_sparse_compat(spg::hip_backend_stream(&g->ctx->be), st.in, va.data(), vb.data(), dst.data(), (int32_t)W, (int64_t)va.size(), need,
                                        ca.data(), cb.data(), sa.data(), sb.data(), n, records, kk, max_d2, pair_max_d2, joint_max_d2, out, &nacc, cs,
                                        g->ctx->err, sizeof g->ctx->err)) return rc;
    if (stats) *stats = cs;
    return nacc;
}
}  // namespace

extern "C" int spg_graph_compatible_candidates(spg_graph *g, int32_t fixed_id, const int32_t *ij, const double *records, int n, int k, double max_d2,
                                               double pair_max_d2, const double *joint_max_d2, int32_t *compatible, double *joint_d2, int cap,
                                               int32_t *clique, int clique_cap, double *d2, int32_t *degree, int32_t *status, double *pair_d2,
                                               int64_t pair_cap, spg_compat_stats *stats) {
    return compat_call(g, fixed_id, ij, records, n, k, max_d2, pair_max_d2, joint_max_d2, compatible, joint_d2, cap, clique, clique_cap, d2, degree, status,
                       pair_d2, pair_cap, stats);
}

extern "C" int spg_ctx_max_clique(spg_ctx *ctx, int n, const uint64_t *adj, int32_t *clique, int cap, int32_t *seed) {
    const char *what = "spg_ctx_max_clique";
    if (!ctx || n < 0) return SPG_EINVAL;
    if (n == 0) return 0;
    if (!adj) return SPG_EINVAL;
    if (n > kCompatMaxN) return fail(ctx, SPG_ECAPACITY, "%s: %d vertices, limited to %d", what, n, kCompatMaxN);
    const int nw = (n + 63) / 64;
    for (int i = 0; i < n; i++)
        for (int w = 0; w < nw; w++) {
            uint64_t bits = adj[(size_t)i * nw + w];
            if (w == nw - 1 && (n & 63) && (bits >> (n & 63))) return fail(ctx, SPG_EINVAL, "%s: row %d has bits at or beyond n", what, i);
            while (bits) {
                const int j = w * 64 + __builtin_ctzll(bits);
                bits &= bits - 1;
                if (j == i) return fail(ctx, SPG_EINVAL, "%s: the diagonal bit of row %d is set", what, i);
                if (!((adj[(size_t)j * nw + (i >> 6)] >> (i & 63)) & 1)) return fail(ctx, SPG_EINVAL, "%s: not symmetric at (%d, %d)", what, i, j);
            }
        }
    if (!ctx->is_hip) return set_err(ctx, SPG_ESTATE, "%s needs the HIP backend", what);
    std::vector<int32_t> members((size_t)n);
    int size = 0;
    int32_t sd = -1;
    if (int rc = spg::hip_max_clique(spg::hip_backend_stream(&ctx->be), n, adj, members.data(), &size, &sd, ctx->err, sizeof ctx->err)) return rc;
    if (clique && cap >= size) std::copy(members.begin(), members.begin() + size, clique);
    if (seed) *seed = sd;
    return size;
}

// ================================================================================= proposal of candidates
// spg_graph_propose_candidates: the argument checks, the live vertices by rank (ascending id) with the CSR of the live
// adjacency over ranks (built from the edge lists as they stand: nothing is renumbered or reordered for stage A), the
// search on the device, and for range > 0 the kept pairs handed to the relative-covariance path with the gate behind it.
extern "C" int64_t spg_graph_propose_candidates(spg_graph *g, int32_t fixed_id, double search_radius, double max_angle, int32_t min_id_gap,
                                                int32_t max_per_vertex, const int32_t *queries, int n_queries, double range, double z_max, int32_t *ij,
                                                double *dist, double *angle, double *sigma, double *zscore, int64_t cap, spg_propose_stats *stats) {
    const char *what = "spg_graph_propose_candidates";
    if (!g || (queries && n_queries < 0)) return SPG_EINVAL;
    spg_ctx *c = g->ctx;
    if (!(search_radius > 0.0) || !std::isfinite(search_radius)) return fail(c, SPG_EINVAL, "%s: search_radius %g must be positive and finite", what, search_radius);
    if (std::isnan(max_angle)) return set_err(c, SPG_EINVAL, "%s: max_angle is not a number", what);
    if (max_per_vertex < 0 || max_per_vertex > 32) return fail(c, SPG_EINVAL, "%s: max_per_vertex %d is outside 0 .. 32", what, (int)max_per_vertex);
    if (std::isnan(range) || range > search_radius) return fail(c, SPG_EINVAL, "%s: range %g must not exceed search_radius %g", what, range, search_radius);
    if (std::isnan(z_max)) return set_err(c, SPG_EINVAL, "%s: z_max is not a number", what);
    if (g->active) return set_err(c, SPG_EINVAL, "%s: a stepwise marginalisation is active", what);
    std::vector<int32_t> order = live_vertices_by_id(g);
    const int n = (int)order.size();
    if (n == 0) return 0;
    const int fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return fail(c, SPG_EINVAL, "%s: the fixed vertex %d is not in the graph", what, (int)fixed_id);
    std::vector<int32_t> rank_of(g->vid.size(), -1), ids((size_t)n), qlist;
    std::vector<int64_t> vpo((size_t)n);
    for (int r = 0; r < n; r++) { rank_of[order[r]] = r; ids[r] = g->vid[order[r]]; vpo[r] = g->vpose[order[r]]; }
    std::vector<uint8_t> isq((size_t)n, queries ? 0 : 1);
    if (queries) {
        for (int i = 0; i < n_queries; i++) {
            const int v = live_index(g, queries[i]);
            if (v < 0) return fail(c, SPG_EINVAL, "%s: query %d: vertex %d is not in the graph", what, i, (int)queries[i]);
            if (isq[rank_of[v]]) return fail(c, SPG_EINVAL, "%s: query %d: vertex %d is listed twice", what, i, (int)queries[i]);
            isq[rank_of[v]] = 1;
        }
    }
    for (int r = 0; r < n; r++) if (isq[r]) qlist.push_back(r);
    spg_propose_stats ps{};
    if (n < 2 || qlist.empty()) { if (stats) *stats = ps; return 0; }
    if (!c->is_hip) return set_err(c, SPG_ESTATE, "%s needs the HIP backend", what);
    int table_bits = -1;
    if (const char *e = getenv("SPG_PROPOSE_TABLE_BITS")) {
        table_bits = atoi(e);
        if (table_bits < 0 || table_bits > 30) return fail(c, SPG_EINVAL, "%s: SPG_PROPOSE_TABLE_BITS=%s is outside 0 .. 30", what, e);
    }
    if (int rc = sync_device(g)) return rc;
    if (int rc = c->be.synchronize(c->be.user)) return rc;
    c->err[0] = 0;
    // rule 4: every two vertices of one live edge are neighbours
    std::vector<std::pair<int32_t, int32_t>> nb;
    for (const GEdge &ge : g->edges) {
        if (!ge.alive) continue;
        const int32_t *vs = edge_verts(g, ge);
        for (int i = 0; i < ge.nv; i++)
            for (int j = 0; j < ge.nv; j++)
                if (i != j && rank_of[vs[i]] >= 0 && rank_of[vs[j]] >= 0) nb.push_back({rank_of[vs[i]], rank_of[vs[j]]});
    }
    std::sort(nb.begin(), nb.end());
    nb.erase(std::unique(nb.begin(), nb.end()), nb.end());
    std::vector<int32_t> adjptr((size_t)n + 1, 0), adj(nb.size());
    for (size_t i = 0; i < nb.size(); i++) { adjptr[(size_t)nb[i].first + 1]++; adj[i] = nb[i].second; }
    for (int r = 0; r < n; r++) adjptr[(size_t)r + 1] += adjptr[r];
    const spg::ProposeIn in{g->d, n, (int)qlist.size(), g->dev, vpo.data(), ids.data(), isq.data(), qlist.data(), adjptr.data(), adj.data(),
                            search_radius, max_angle, (int)min_id_gap, (int)max_per_vertex, table_bits};
    const bool gate = range > 0.0, room = ij && dist && angle;
    std::vector<int32_t> pij;
    std::vector<double> pdist, pangle;
    void *stream = spg::hip_backend_stream(&c->be);
    // without the gate a call that cannot write asks for the count alone
    if (int rc = spg::hip_propose_search(stream, in, gate || room, pij, pdist, pangle, ps, c->err, sizeof c->err)) return rc;
    int64_t count = ps.n_kept;
    ps.n_gated = count;
    if (!gate) {
        if (stats) *stats = ps;
        if (!room || cap < count) return count;
        std::copy(pij.begin(), pij.end(), ij);
        std::copy(pdist.begin(), pdist.end(), dist);
        std::copy(pangle.begin(), pangle.end(), angle);
        return count;
    }
    std::vector<double> sg((size_t)count), zs((size_t)count);
    if (count > 0) {
        const int D = g->d;
        const int64_t W = 2 * D;
        std::vector<int32_t> va, vb, ca((size_t)count), cb((size_t)count), slot((size_t)count);
        std::vector<int64_t> dst;
        for (int64_t i = 0; i < count; i++) {   // the pairs are distinct: one block each, laid out as relative_call lays them
            const int32_t v[2] = {g->index_of(pij[2 * i]), g->index_of(pij[2 * i + 1])};
            for (int ka = 0; ka < 2; ka++)
                for (int kb = 0; kb < 2; kb++) { va.push_back(v[ka]); vb.push_back(v[kb]); dst.push_back(i * W * W + ka * D * W + kb * D); }
            ca[i] = v[0]; cb[i] = v[1]; slot[i] = (int32_t)i;
        }
        DenseStage st;
        const int64_t blocks_len = count * W * W;
        const int staged = cov_stage(g, fixed, order, {&va, &vb}, blocks_len, nullptr, what, st);
        if (staged < 0) return staged;
        if (int rc = spg::hip_propose_gate(stream, st.in, va.data(), vb.data(), dst.data(), (int32_t)W, (int64_t)va.size(), blocks_len, ca.data(), cb.data(),
                                           slot.data(), (int)count, range, sg.data(), zs.data(), ps.solve, c->err, sizeof c->err)) return rc;
    }
    std::vector<int64_t> pass;
    for (int64_t i = 0; i < count; i++) if (zs[i] <= z_max || zs[i] <= 0.0) pass.push_back(i);   // zscore <= 0: rho <= range, passes whatever z_max
    ps.n_gated = (int64_t)pass.size();
    if (stats) *stats = ps;
    if (!room || cap < ps.n_gated) return ps.n_gated;
    for (size_t k = 0; k < pass.size(); k++) {
        const int64_t i = pass[k];
        ij[2 * k] = pij[2 * i]; ij[2 * k + 1] = pij[2 * i + 1];
        dist[k] = pdist[i]; angle[k] = pangle[i];
        if (sigma) sigma[k] = sg[i];
        if (zscore) zscore[k] = zs[i];
    }
    return ps.n_gated;
}

// ================================================================================= selection of removals
// spg_graph_select_removals: the argument checks, the total order of the live vertices (the keep list, then a sort by
// priority or by the hashed id), the decision on the device.
namespace {
inline uint64_t mix64(uint64_t k) {   // the splitmix64 finaliser, the constants of pp_hash
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return k;
}
}  // namespace

extern "C" int64_t spg_graph_select_removals(spg_graph *g, double radius, double max_angle, const int32_t *keep, int n_keep, const double *priority,
                                             int32_t *removed, int32_t *representative, double *rep_dist, int64_t cap, spg_removal_stats *stats) {
    const char *what = "spg_graph_select_removals";
    if (!g || n_keep < 0 || (n_keep > 0 && !keep)) return SPG_EINVAL;
    spg_ctx *c = g->ctx;
    if (!(radius > 0.0) || !std::isfinite(radius)) return fail(c, SPG_EINVAL, "%s: radius %g must be positive and finite", what, radius);
    if (std::isnan(max_angle)) return set_err(c, SPG_EINVAL, "%s: max_angle is not a number", what);
    if (g->active) return set_err(c, SPG_EINVAL, "%s: a stepwise marginalisation is active", what);
    std::vector<int32_t> order = live_vertices_by_id(g);
    const int n = (int)order.size();
    std::vector<int32_t> rank_of(g->vid.size(), -1), ids((size_t)n);
    std::vector<int64_t> vpo((size_t)n);
    for (int r = 0; r < n; r++) { rank_of[order[r]] = r; ids[r] = g->vid[order[r]]; vpo[r] = g->vpose[order[r]]; }
    constexpr uint32_t kNoPlace = ~0u;
    std::vector<uint32_t> pos((size_t)n, kNoPlace);
    for (int i = 0; i < n_keep; i++) {
        const int v = live_index(g, keep[i]);
        if (v < 0) return fail(c, SPG_EINVAL, "%s: keep %d: vertex %d is not in the graph", what, i, (int)keep[i]);
        if (pos[rank_of[v]] != kNoPlace) return fail(c, SPG_EINVAL, "%s: keep %d: vertex %d is listed twice", what, i, (int)keep[i]);
        pos[rank_of[v]] = (uint32_t)i;
    }
    if (priority)
        for (int r = 0; r < n; r++)
            if (std::isnan(priority[r])) return fail(c, SPG_EINVAL, "%s: the priority of vertex %d is not a number", what, (int)ids[r]);
    spg_removal_stats rs{};
    rs.n_live = n; rs.n_forced = n_keep; rs.n_kept = n;
    if (n < 2) { if (stats) *stats = rs; return 0; }
    if (!c->is_hip) return set_err(c, SPG_ESTATE, "%s needs the HIP backend", what);
    int table_bits = -1;
    if (const char *e = getenv("SPG_PROPOSE_TABLE_BITS")) {
        table_bits = atoi(e);
        if (table_bits < 0 || table_bits > 30) return fail(c, SPG_EINVAL, "%s: SPG_PROPOSE_TABLE_BITS=%s is outside 0 .. 30", what, e);
    }
    // the unforced ranks in order; rank order is id order, so the rank breaks the ties
    std::vector<int32_t> rest;
    for (int r = 0; r < n; r++) if (pos[r] == kNoPlace) rest.push_back(r);
    if (priority) {
        std::sort(rest.begin(), rest.end(), [&](int32_t x, int32_t y) { return priority[x] > priority[y] || (priority[x] == priority[y] && x < y); });
    } else {
        std::vector<uint64_t> key((size_t)n);
        for (int r = 0; r < n; r++) key[r] = mix64((uint64_t)(uint32_t)ids[r]);
        std::sort(rest.begin(), rest.end(), [&](int32_t x, int32_t y) { return key[x] < key[y] || (key[x] == key[y] && x < y); });
    }
    for (size_t k = 0; k < rest.size(); k++) pos[rest[k]] = (uint32_t)(n_keep + (int)k);
    if (int rc = sync_device(g)) return rc;
    if (int rc = c->be.synchronize(c->be.user)) return rc;
    c->err[0] = 0;
    const spg::RemovalsIn in{g->d, n, n_keep, g->dev, vpo.data(), ids.data(), pos.data(), radius, max_angle, table_bits};
    const bool room = removed && representative && rep_dist;
    std::vector<int32_t> rem, rep;
    std::vector<double> rd;
    if (int rc = spg::hip_select_removals(spg::hip_backend_stream(&c->be), in, room, rem, rep, rd, rs, c->err, sizeof c->err)) return rc;
    if (stats) *stats = rs;
    const int64_t count = rs.n_removed;
    if (!room || cap < count) return count;
    std::copy(rem.begin(), rem.end(), removed);
    std::copy(rep.begin(), rep.end(), representative);
    std::copy(rd.begin(), rd.end(), rep_dist);
    return count;
}

// ================================================================================= greedy edge pruning, outlier detection
namespace {
// What spg_graph_prune_candidates and spg_graph_detect_outliers share. Candidate i is live edge edge_idx[i] in the order
// of spg_graph_get_edges, which is the order of the staged edge list; the endpoint set, its joint covariance and the slots
// are built as in select_call. `outputs`: the caller's ordered arrays are there (else the size query). run(in, va, vb,
// dst, ld, nblk, len, sa, sb, kk, m, lazy) is the device call: it resets its stats for m endpoints and writes the number
// chosen to `count`. `ran` is set when a device call succeeded: the return value is then `count`, and the caller's stats
// are those of the result (a size query, n = 0 or k = 0 and every error leave it false).
template <class Run>
int edge_greedy_call(spg_graph *g, const char *what, int32_t fixed_id, const int32_t *edge_idx, int n, int k, bool outputs, int cap, const int &count,
                     bool &ran, Run run) {
    ran = false;
    if (!g || n < 0 || (n > 0 && !edge_idx)) return SPG_EINVAL;
    if (k < 0) return set_err(g->ctx, SPG_EINVAL, "%s: k is negative", what);
    if (g->active) return set_err(g->ctx, SPG_EINVAL, "%s: a stepwise marginalisation is active", what);
    std::vector<int32_t> order = live_vertices_by_id(g);
    const int fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return set_err(g->ctx, SPG_EINVAL, "%s: the fixed vertex is not in the graph", what);
    const int D = g->d;
    canonicalize_edge_order(g);
    std::vector<int32_t> live;
    live.reserve((size_t)g->n_live_e);
    for (size_t e = 0; e < g->edges.size(); e++) if (g->edges[e].alive) live.push_back((int32_t)e);
    std::vector<int32_t> S, sa((size_t)n), sb((size_t)n);
    std::unordered_map<int32_t, int32_t> slot_of;
    std::unordered_set<int32_t> seen;
    for (int i = 0; i < n; i++) {
        const int32_t x = edge_idx[i];
        const GEdge *ge = (x >= 0 && (size_t)x < live.size()) ? &g->edges[live[x]] : nullptr;
        const char *why = !ge ? "is out of range" : (ge->kind != SPG_EDGE_BINARY || ge->nv != 2) ? "is not a binary edge"
                          : ge->vtx[0] == ge->vtx[1] ? "joins a vertex to itself" : !seen.insert(x).second ? "is listed twice" : nullptr;
        if (why) {
            snprintf(g->ctx->err, sizeof g->ctx->err, "%s: candidate %d: edge %d %s", what, i, (int)x, why);
            return SPG_EINVAL;
        }
        int32_t sl[2];
        for (int e = 0; e < 2; e++) {
            if (ge->vtx[e] == fixed) { sl[e] = -1; continue; }
            auto it = slot_of.emplace(ge->vtx[e], (int32_t)S.size());
            if (it.second) S.push_back(ge->vtx[e]);
            sl[e] = it.first->second;
        }
        sa[i] = sl[0]; sb[i] = sl[1];
    }
    const int kk = std::min(k, n);
    if (kk == 0) return 0;
    const int64_t m = (int64_t)S.size(), W = m * D, need = W * W;
    const int method = g->ctx->greedy_method;
    if (method == SPG_GREEDY_JOINT && W > 46000) {
        snprintf(g->ctx->err, sizeof g->ctx->err, "%s: %lld distinct endpoints, limited to 46k variables, the bound of spg_graph_joint_marginal_covariance",
                 what, (long long)m);
        return SPG_ECAPACITY;
    }
    if (!outputs || cap < kk) return kk;
    if (method == SPG_GREEDY_JOINT || (method == SPG_GREEDY_AUTO && W <= 46000)) {
        std::vector<int32_t> va, vb;
        std::vector<int64_t> dst;
        va.reserve((size_t)(m * m)); vb.reserve((size_t)(m * m)); dst.reserve((size_t)(m * m));
        for (int64_t a = 0; a < m; a++)
            for (int64_t b = 0; b < m; b++) { va.push_back(S[a]); vb.push_back(S[b]); dst.push_back(a * D * W + b * D); }
        DenseStage st;
        const int staged = cov_stage(g, fixed, order, {&va, &vb}, need, nullptr, what, st);
        if (staged < 0) return staged;
        const int rc = run(st.in, va.data(), vb.data(), dst.data(), (int32_t)W, (int64_t)va.size(), need, sa.data(), sb.data(), kk, (int32_t)m,
                           (const spg::GreedyLazyIn *)nullptr);
        if (rc == 0) {
            joint_greedy_stats(g->ctx, count);
            ran = true;
            return count;
        }
        if (!(method == SPG_GREEDY_AUTO && rc == SPG_ECAPACITY)) return rc;   // AUTO: what JOINT cannot hold goes to LAZY
    }
    PairBlocks pb;   // every pair is an edge: its block lies in the fronts of the selected inverse
    for (int i = 0; i < n; i++) { const GEdge &ge = g->edges[live[edge_idx[i]]]; pb.add(ge.vtx[0], ge.vtx[1], D); }
    DenseStage st;
    const int staged = cov_stage(g, fixed, order, {&pb.va, &pb.vb}, pb.len(D), nullptr, what, st);
    if (staged < 0) return staged;
    const spg::GreedyLazyIn lz{pb.slot.data(), S.data(), (int)m, g->ctx->greedy_lookahead, &g->ctx->greedy_stats};
    if (int rc = run(st.in, pb.va.data(), pb.vb.data(), pb.dst.data(), (int32_t)(2 * D), (int64_t)pb.va.size(), pb.len(D), sa.data(), sb.data(), kk,
                     (int32_t)m, &lz)) return rc;
    ran = true;
    return count;
}
}  // namespace

extern "C" int spg_graph_prune_candidates(spg_graph *g, int32_t fixed_id, const int32_t *edge_idx, int n, int k, double max_loss, double max_kld,
                                          double min_margin, int32_t *pruned, double *cond_loss, double *kld, int cap, double *final_loss,
                                          double *final_margin, int32_t *status, spg_prune_stats *stats) {
    spg_prune_stats ps{};
    int npruned = 0;
    bool ran = false;
    const double margin = min_margin > 0.0 ? min_margin : 1e-6;
    const int r = edge_greedy_call(
        g, "spg_graph_prune_candidates", fixed_id, edge_idx, n, k, pruned && cond_loss && kld, cap, npruned, ran,
        [&](const spg::DenseGraphIn &in, const int32_t *va, const int32_t *vb, const int64_t *dst, int32_t ld, int64_t nblk, int64_t len, const int32_t *sa,
            const int32_t *sb, int kk, int32_t m, const spg::GreedyLazyIn *lz) {
            ps = spg_prune_stats{};
            ps.endpoints = m;
            return spg::hip_sparse_prune(spg::hip_backend_stream(&g->ctx->be), in, va, vb, dst, ld, nblk, len, edge_idx, sa, sb, n, kk, max_loss, max_kld,
                                         margin, pruned, cond_loss, kld, final_loss, final_margin, status, &npruned, ps, g->ctx->err, sizeof g->ctx->err, lz);
        });
    if (ran && stats) *stats = ps;
    return r;
}

extern "C" int spg_graph_detect_outliers(spg_graph *g, int32_t fixed_id, const int32_t *edge_idx, int n, int k, double min_stat, double min_margin,
                                         int32_t *flagged, double *stat, int cap, double *final_stat, double *final_margin, double *redundancy,
                                         int32_t *status, spg_outlier_stats *stats) {
    spg_outlier_stats os{};
    int nflagged = 0;
    bool ran = false;
    const double margin = min_margin > 0.0 ? min_margin : 1e-6;
    const int r = edge_greedy_call(
        g, "spg_graph_detect_outliers", fixed_id, edge_idx, n, k, flagged && stat, cap, nflagged, ran,
        [&](const spg::DenseGraphIn &in, const int32_t *va, const int32_t *vb, const int64_t *dst, int32_t ld, int64_t nblk, int64_t len, const int32_t *sa,
            const int32_t *sb, int kk, int32_t m, const spg::GreedyLazyIn *lz) {
            os = spg_outlier_stats{};
            os.endpoints = m;
            return spg::hip_sparse_detect(spg::hip_backend_stream(&g->ctx->be), in, va, vb, dst, ld, nblk, len, edge_idx, sa, sb, n, kk, min_stat, margin,
                                          flagged, stat, final_stat, final_margin, redundancy, status, &nflagged, os, g->ctx->err, sizeof g->ctx->err, lz);
        });
    if (ran && stats) *stats = os;
    return r;
}

// ================================================================================= robust kernel
namespace {
// The graph's kernel into a staged graph: kind, width and, per live edge in the stage's order, whether it applies — a
// binary edge between two different vertices whose ids are at least robust_gap apart. `elig` must outlive st.in.
void stage_robust(const spg_graph *g, DenseStage &st, std::vector<uint8_t> &elig) {
    if (g->robust_kind == SPG_ROBUST_NONE) return;
    elig.assign(st.er.size(), 0);
    for (size_t e = 0; e < st.er.size(); e++) {
        if (st.er[e].kind != SPG_EDGE_BINARY) continue;
        const int32_t vi = st.ev[st.er[e].vbegin], vj = st.ev[st.er[e].vbegin + 1];
        const int64_t gap = std::llabs((int64_t)g->vid[vi] - (int64_t)g->vid[vj]);
        elig[e] = vi != vj && gap >= g->robust_gap;
    }
    st.in.robust_kind = g->robust_kind; st.in.robust_delta = g->robust_delta; st.in.robust_elig = elig.data();
}
}  // namespace

extern "C" int spg_graph_set_robust_kernel(spg_graph *g, int kind, double delta, int min_id_gap) {
    if (!g || g->active || kind < SPG_ROBUST_NONE || kind > SPG_ROBUST_DCS) return SPG_EINVAL;
    if (kind != SPG_ROBUST_NONE && !(std::isfinite(delta) && delta > 0)) return SPG_EINVAL;
    g->robust_kind = kind;
    if (kind != SPG_ROBUST_NONE) g->robust_delta = delta;
    g->robust_gap = std::max(min_id_gap, 1);
    return 0;
}

extern "C" int spg_graph_get_robust_kernel(const spg_graph *g, int *kind, double *delta, int *min_id_gap) {
    if (!g) return SPG_EINVAL;
    if (kind) *kind = g->robust_kind;
    if (delta) *delta = g->robust_delta;
    if (min_id_gap) *min_id_gap = g->robust_gap;
    return 0;
}

extern "C" int spg_graph_edge_chi2(spg_graph *g, double *chi2, double *rho, double *weight, int cap) {
    if (!g || g->active) return SPG_EINVAL;
    const int ne = g->n_live_e;
    if (cap < ne || !(chi2 || rho || weight)) return ne;
    if (!g->ctx->is_hip) return set_err(g->ctx, SPG_ESTATE, "spg_graph_edge_chi2 needs the HIP backend");
    if (ne == 0) return 0;
    // nothing is a variable: only the errors are evaluated. The stage lists the live edges in spg_graph_get_edges order.
    DenseStage st;
    if (int rc = stage_global(g, {}, {}, g->d, st)) return rc;
    std::vector<uint8_t> elig;
    stage_robust(g, st, elig);
    int rc = spg::hip_edge_chi2(spg::hip_backend_stream(&g->ctx->be), st.in, chi2, rho, weight, g->ctx->err, sizeof g->ctx->err);
    return rc ? rc : ne;
}

// ================================================================================= optimize() (8f.1)
// robust: honour the graph's kernel (spg_graph_chi2 does not)
static int optimize_with_fixed(spg_graph *g, int iterations, const std::vector<int32_t> &fixed_vertices, spg_optimize_stats *out, bool robust = true) {
    spg_ctx *ctx = g->ctx;
    std::vector<int32_t> order = live_vertices_by_id(g);
    std::vector<uint8_t> is_fixed(g->vid.size(), 0);
    for (int32_t v : fixed_vertices) is_fixed[v] = 1;
    int64_t n = 0;
    for (int32_t v : order) if (!is_fixed[v]) n += g->d;
    // dense up to 12 k unknowns (two n^2 matrices, an n^3 / 3 factorisation per trial), block-sparse beyond; conjugate
    // gradients on the block-CSR matrix only on request
    const bool pcg = ctx->linear_solver == SPG_SOLVER_PCG && n > 0;
    const bool sparse = ctx->linear_solver == SPG_SOLVER_SPARSE || (ctx->linear_solver == SPG_SOLVER_AUTO && n > 12000);
    if (!sparse && !pcg && n > 32000) return set_err(ctx, SPG_ECAPACITY, "spg_graph_optimize: dense formulation limited to 32k variables (2 x 8 GB)");
    DenseStage st;
    if (int rc = stage_global(g, order, fixed_vertices, g->d, st)) return rc;
    std::vector<uint8_t> elig;
    if (robust) stage_robust(g, st, elig);
    spg_optimize_stats os{};
    os.n = n;
    os.solver = pcg ? SPG_SOLVER_PCG : (sparse && n > 0) ? SPG_SOLVER_SPARSE : SPG_SOLVER_DENSE;
    ctx->pcg_stats = spg_pcg_stats{};
    int rc;
    if (pcg) {
        spg::bsr::Pattern P;
        spg::bsr::build_pattern(st.in.nv, st.in.pos, g->d, st.in.ne, st.in.er, st.in.ev, P);
        const double rel_tol = ctx->pcg_rel_tol > 0 ? ctx->pcg_rel_tol : 1e-10;
        const int max_iter = ctx->pcg_max_iter > 0 ? ctx->pcg_max_iter : (int)std::min<int64_t>(n, 20000);
        rc = spg::hip_pcg_optimize(spg::hip_backend_stream(&ctx->be), st.in, P, (int)n, iterations, rel_tol, max_iter, os, ctx->pcg_stats,
                                   ctx->err, sizeof ctx->err);
    } else {
        auto *run = os.solver == SPG_SOLVER_SPARSE ? spg::hip_sparse_optimize : spg::hip_dense_optimize;
        rc = run(spg::hip_backend_stream(&ctx->be), st.in, (int)n, iterations, os, ctx->err, sizeof ctx->err);
    }
    // the estimates changed on the device: refresh the host mirror's copies
    if (int rc2 = sync_host(g)) return rc2;
    {
        // one download of the arena range that holds the free vertices' poses (a copy per vertex costs ~30 us each:
        // 3 s for a 100 k-pose graph), then only the pose slots are taken over
        int64_t lo = INT64_MAX, hi = -1;
        for (int32_t v : order) if (!is_fixed[v]) { lo = std::min(lo, g->vpose[v]); hi = std::max(hi, g->vpose[v] + g->ps); }
        if (hi > lo) {
            std::vector<double> tmp((size_t)(hi - lo));
            if (int rc2 = ctx->be.download(ctx->be.user, tmp.data(), (char *)g->dev + lo * 8, hi - lo)) return rc2;
            for (int32_t v : order) if (!is_fixed[v]) memcpy(g->host.data() + g->vpose[v], tmp.data() + (g->vpose[v] - lo), (size_t)g->ps * 8);
        }
    }
    if (rc) return rc;
    if (out) *out = os;
    return 0;
}

extern "C" int spg_sparse_plan(int n, const int32_t *ptr, const int32_t *adj, int pose_dim, const uint8_t *is_marg, int leaf,
                               spg_sparse_plan_info *info, int32_t *perm, int32_t *sn_first, int32_t *sn_parent, int32_t *sn_level,
                               int32_t *sn_rowptr, int32_t *rows, int32_t *rel, int64_t rows_cap) {
    if (n < 0 || !ptr || (pose_dim != 3 && pose_dim != 6) || !info) return SPG_EINVAL;
    // the row pointers come from the caller: 0-based, non-decreasing, non-negative total — before anything is read through them
    if (ptr[0] != 0) return SPG_EINVAL;
    for (int i = 0; i < n; i++) if (ptr[i + 1] < ptr[i]) return SPG_EINVAL;
    if (!adj && ptr[n] > 0) return SPG_EINVAL;
    spg::sparse::BlockGraph bg;
    bg.n = n;
    bg.ptr.assign(ptr, ptr + n + 1);
    bg.adj.assign(adj, adj + ptr[n]);
    for (int32_t u : bg.adj) if (u < 0 || u >= n) return SPG_EINVAL;
    spg::sparse::Plan P;
    spg::sparse::build_plan(bg, pose_dim, is_marg, leaf > 0 ? leaf : (pose_dim == 6 ? 32 : 64), P);
    info->n_supernodes = P.nsn; info->n_marg_supernodes = P.n_marg_sn; info->n_levels = P.nlevels; info->pad_ = 0;
    info->n_rows = (int64_t)P.rows.size(); info->front_bytes = 8.0 * (double)P.pool; info->flops = P.flops;
    if (perm) std::copy(P.perm.begin(), P.perm.end(), perm);
    if (sn_first) std::copy(P.first.begin(), P.first.end(), sn_first);
    if (sn_parent) std::copy(P.parent.begin(), P.parent.end(), sn_parent);
    if (sn_level) std::copy(P.level.begin(), P.level.end(), sn_level);
    if (sn_rowptr) std::copy(P.rowptr.begin(), P.rowptr.end(), sn_rowptr);
    if (rows_cap >= (int64_t)P.rows.size()) {
        if (rows) std::copy(P.rows.begin(), P.rows.end(), rows);
        if (rel) std::copy(P.rel.begin(), P.rel.end(), rel);
    }
    return 0;
}

extern "C" int spg_graph_optimize(spg_graph *g, int iterations, int32_t fixed_id, spg_optimize_stats *out) {
    if (!g || g->active || iterations < 0) return SPG_EINVAL;
    if (!g->ctx->is_hip) return set_err(g->ctx, SPG_ESTATE, "spg_graph_optimize needs the HIP backend");
    std::vector<int32_t> order = live_vertices_by_id(g);
    int fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return set_err(g->ctx, SPG_EINVAL, "spg_graph_optimize: the fixed vertex is not in the graph");
    if (order.size() < 2) return set_err(g->ctx, SPG_EINVAL, "spg_graph_optimize: nothing to optimise");
    return optimize_with_fixed(g, iterations, std::vector<int32_t>{(int32_t)fixed}, out);
}

extern "C" int spg_graph_optimize_fixed(spg_graph *g, int iterations, const int32_t *fixed_ids, int n_fixed, spg_optimize_stats *out) {
    if (!g || g->active || iterations < 0 || n_fixed < 0 || (n_fixed > 0 && !fixed_ids)) return SPG_EINVAL;
    if (!g->ctx->is_hip) return set_err(g->ctx, SPG_ESTATE, "spg_graph_optimize_fixed needs the HIP backend");
    std::vector<int32_t> fx;
    for (int i = 0; i < n_fixed; i++) {
        auto it = g->vidx.find(fixed_ids[i]);
        if (it == g->vidx.end() || !g->valive[it->second]) return set_err(g->ctx, SPG_EINVAL, "spg_graph_optimize_fixed: a fixed vertex is not in the graph");
        fx.push_back(it->second);
    }
    return optimize_with_fixed(g, iterations, fx, out);
}

// zero iterations with every vertex fixed: the optimiser's entry evaluates chi2 and returns
static int graph_chi2(spg_graph *g, double *chi2) {
    std::vector<int32_t> all;
    for (size_t i = 0; i < g->vid.size(); i++) if (g->valive[i]) all.push_back((int32_t)i);
    spg_optimize_stats st{};
    int rc = optimize_with_fixed(g, 1, all, &st, false);
    if (rc) return rc;
    *chi2 = st.chi2_initial;
    return 0;
}

extern "C" int spg_graph_chi2(spg_graph *g, double *chi2) {
    if (!g || !chi2 || g->active) return SPG_EINVAL;
    if (!g->ctx->is_hip) return set_err(g->ctx, SPG_ESTATE, "spg_graph_chi2 needs the HIP backend");
    return graph_chi2(g, chi2);
}

// ================================================================================= initialize()
namespace {
// Breadth-first spanning tree over the binary edges from `fixed` (spg_graph_initialize in include/spg.h states the
// tie-breaks): level[v] (-1 = not reached), and tree = the composed pose of every reached vertex, indexed by vertex
// (pose stride apart), the fixed one's taken from the host mirror. Counts the edges that enter and those that do not.
struct SpanningTree {
    std::vector<int32_t> level;
    std::vector<double> tree;
    int depth = 0, used = 0, ignored = 0;
};
bool enters_initialize(const GEdge &ge) { return ge.alive && ge.kind == SPG_EDGE_BINARY && ge.nv == 2 && ge.vtx[0] != ge.vtx[1]; }

void build_spanning_tree(const spg_graph *g, int fixed, SpanningTree &T) {
    const double PI = 3.14159265358979323846;
    const int d = g->d, ps = g->ps;
    const size_t nv = g->vid.size();
    for (const GEdge &ge : g->edges) if (ge.alive) (enters_initialize(ge) ? T.used : T.ignored)++;
    T.level.assign(nv, -1);
    T.tree.assign(nv * ps, 0.0);
    std::vector<int32_t> parent(nv, -1), pedge(nv, -1), frontier{(int32_t)fixed}, next;
    T.level[fixed] = 0;
    memcpy(T.tree.data() + (size_t)fixed * ps, g->host.data() + g->vpose[fixed], (size_t)ps * 8);
    for (int L = 0; !frontier.empty(); L++) {
        T.depth = L;
        next.clear();
        for (int32_t v : frontier)
            for (const auto &a : g->vr[v].adj) {
                const GEdge &ge = g->edges[a.eid];
                if (!enters_initialize(ge)) continue;
                const int32_t u = ge.vtx[0] == v ? ge.vtx[1] : ge.vtx[0];
                if (T.level[u] < 0) { T.level[u] = L + 1; next.push_back(u); parent[u] = v; pedge[u] = a.eid; }
                else if (T.level[u] == L + 1 &&
                         (g->vid[v] < g->vid[parent[u]] || (v == parent[u] && a.eid < pedge[u]))) { parent[u] = v; pedge[u] = a.eid; }
            }
        // every parent of the level is final: compose
        for (int32_t u : next) {
            const GEdge &ge = g->edges[pedge[u]];
            const double *Z = g->host.data() + ge.off, *Tp = T.tree.data() + (size_t)parent[u] * ps;
            double *Tc = T.tree.data() + (size_t)u * ps, zi[7];
            if (ge.vtx[0] == parent[u]) pose_compose(d, Tp, Z, Tc);
            else { pose_inverse(d, Z, zi); pose_compose(d, Tp, zi, Tc); }
            if (d == 3) { if (Tc[2] <= -PI) Tc[2] += 2 * PI; }
            else if (Tc[6] < 0) for (int i = 3; i < 7; i++) Tc[i] = -Tc[i];
        }
        frontier.swap(next);
    }
}

// mean diagonal of the rotation (rot = true) or translation block of a binary edge's information
double init_weight(int d, const double *rec, bool rot) {
    const int ps = pose_stride(d);
    auto dg = [&](int i) { return rec[ps + i * d - i * (i - 1) / 2]; };
    if (d == 6) return rot ? (dg(3) + dg(4) + dg(5)) / 3.0 : (dg(0) + dg(1) + dg(2)) / 3.0;
    return rot ? dg(2) : (dg(0) + dg(1)) / 2.0;
}

}  // namespace

extern "C" int spg_graph_initialize(spg_graph *g, int method, int32_t fixed_id, spg_init_stats *out) {
    if (!g || g->active) return SPG_EINVAL;
    spg_ctx *ctx = g->ctx;
    if (method != SPG_INIT_SPANNING_TREE && method != SPG_INIT_CHORDAL) return set_err(ctx, SPG_EINVAL, "spg_graph_initialize: unknown method");
    std::vector<int32_t> order = live_vertices_by_id(g);
    const int fixed = resolve_fixed(g, order, fixed_id);
    if (fixed < 0) return set_err(ctx, SPG_EINVAL, "spg_graph_initialize: the fixed vertex is not in the graph");
    if (method == SPG_INIT_CHORDAL && !ctx->is_hip) return set_err(ctx, SPG_ESTATE, "spg_graph_initialize: SPG_INIT_CHORDAL needs the HIP backend");
    canonicalize_edge_order(g);
    if (int rc = sync_host(g)) return rc;
    SpanningTree T;
    build_spanning_tree(g, fixed, T);
    for (int32_t v : order)
        if (T.level[v] < 0) {
            snprintf(ctx->err, sizeof ctx->err, "spg_graph_initialize: vertex %d is not reachable from the fixed vertex %d over binary edges",
                     (int)g->vid[v], (int)g->vid[fixed]);
            return SPG_EINVAL;
        }
    if (method == SPG_INIT_CHORDAL)
        for (const GEdge &ge : g->edges) {
            if (!enters_initialize(ge)) continue;
            const double kappa = init_weight(g->d, g->host.data() + ge.off, true), tau = init_weight(g->d, g->host.data() + ge.off, false);
            if (!(std::isfinite(kappa) && std::isfinite(tau) && kappa > 0 && tau > 0)) {
                snprintf(ctx->err, sizeof ctx->err, "spg_graph_initialize: edge (%d, %d) has a rotation or translation weight that is not finite and positive",
                         (int)g->vid[ge.vtx[0]], (int)g->vid[ge.vtx[1]]);
                return SPG_EINVAL;
            }
        }
    spg_init_stats is{};
    is.method = method; is.n_vertices = (int32_t)order.size(); is.edges_used = T.used; is.edges_ignored = T.ignored; is.tree_depth = T.depth;
    is.chi2_before = is.chi2_after = std::nan("");
    if (ctx->is_hip) if (int rc = graph_chi2(g, &is.chi2_before)) return rc;
    if (order.size() > 1) {
        // the arena range that holds the free vertices' poses
        int64_t lo = INT64_MAX, hi = -1;
        for (int32_t v : order) if (v != fixed) { lo = std::min(lo, g->vpose[v]); hi = std::max(hi, g->vpose[v] + g->ps); }
        if (method == SPG_INIT_SPANNING_TREE) {
            if (int rc = ctx->be.synchronize(ctx->be.user)) return rc;
            for (int32_t v : order) if (v != fixed) memcpy(g->host.data() + g->vpose[v], T.tree.data() + (size_t)v * g->ps, (size_t)g->ps * 8);
            // one upload of that range as far as the device holds it (the rest follows with the next sync_device)
            const int64_t top = std::min(hi, g->dev_synced);
            if (g->dev && top > lo)
                if (int rc = ctx->be.upload(ctx->be.user, (char *)g->dev + lo * 8, g->host.data() + lo, top - lo)) return rc;
        } else {
            DenseStage st;
            if (int rc = stage_global(g, order, {(int32_t)fixed}, 1, st)) return rc;
            if (int rc = spg::hip_chordal_init(spg::hip_backend_stream(&ctx->be), st.in, fixed, T.tree.data(), is, ctx->err, sizeof ctx->err)) return rc;
            std::vector<double> tmp((size_t)(hi - lo));
            if (int rc = ctx->be.download(ctx->be.user, tmp.data(), (char *)g->dev + lo * 8, hi - lo)) return rc;
            for (int32_t v : order) if (v != fixed) memcpy(g->host.data() + g->vpose[v], tmp.data() + (g->vpose[v] - lo), (size_t)g->ps * 8);
        }
    }
    if (ctx->is_hip) if (int rc = graph_chi2(g, &is.chi2_after)) return rc;
    if (out) *out = is;
    return 0;
}
