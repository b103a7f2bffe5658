// csrc/spg_host.cpp — host side of libspg_hip.so: contexts, the device-resident pose graph, its I/O and the
// self-contained calls of the C ABI of include/spg.h. The marginalisation drivers have their own units:
// spg_host_rounds.cpp (round scheduler, batch driver) and spg_host_stream.cpp (streaming driver).
//
// What stays on the host is the integer graph work of the reference's loop:
//   markovBlanketVertices / extendedMarkovBlanketVertices / markovBlanketEdges
//                                             src/vertex_remover.cpp:142-251
//   buildSubgraph's vertex ordering           src/vertex_remover.cpp:349-356
//   updateInputGraph                          src/vertex_remover.cpp:500-546
//   GraphWrapperG2O bookkeeping               src/graph_wrapper_g2o.cpp:207-247,398-453
// Everything numeric runs in the HIP backend (spg_hip_backend.cpp, kernels in spg_kernels.hip) on records that live in one HBM
// arena: [poses | edge records | per-round output regions]. The host keeps topology only.
#include "spg_graph_impl.h"

// ================================================================================= context
// SPG_SEGV_BACKTRACE=1 (diagnostic): a SIGSEGV inside the process prints the native frames (addresses relative to the
// load address of this library, for addr2line on a -g build) before the default action runs.
#if defined(__linux__)
#include <execinfo.h>
#include <signal.h>
#include <dlfcn.h>
static void spg_segv_handler(int sig) {
    void *frames[64];
    const int n = backtrace(frames, 64);
    Dl_info di;
    const char *base = nullptr;
    if (dladdr((void *)&spg_segv_handler, &di)) base = (const char *)di.dli_fbase;
    char line[160];
    int len = snprintf(line, sizeof line, "spg: signal %d; frames relative to libspg_hip.so (base %p):\n", sig, (const void *)base);
    if (write(2, line, (size_t)len) < 0) {}
    for (int i = 0; i < n; i++) {
        Dl_info fi;
        const bool ours = dladdr(frames[i], &fi) && fi.dli_fbase == (void *)base;
        len = snprintf(line, sizeof line, "  #%d %s0x%llx\n", i, ours ? "+" : "abs ", (unsigned long long)(ours ? (const char *)frames[i] - base : (const char *)frames[i] - (const char *)0));
        if (write(2, line, (size_t)len) < 0) {}
    }
    signal(sig, SIG_DFL);
    raise(sig);
}
static void spg_install_segv_trace() {
    static bool done = false;
    const char *e = getenv("SPG_SEGV_BACKTRACE");
    if (done || !(e && e[0] == '1')) return;
    done = true;
    signal(SIGSEGV, spg_segv_handler);
    signal(SIGABRT, spg_segv_handler);
}
#else
static void spg_install_segv_trace() {}
#endif

extern "C" int spg_ctx_create(spg_ctx **out, int device) {
    spg_install_segv_trace();
    if (!out) return SPG_EINVAL;
    spg_ctx *c = new spg_ctx;
    int rc = spg::hip_backend_create(device, &c->be, c->err, sizeof c->err);
    if (rc != 0) {
        fprintf(stderr, "libspg_hip: %s\n", c->err);
        delete c;
        *out = nullptr;
        return rc;
    }
    c->is_hip = true;
    *out = c;
    return 0;
}

extern "C" int spg_ctx_create_injected(spg_ctx **out, const spg_backend *backend) {
    if (!out || !backend || !backend->alloc || !backend->run_round) return SPG_EINVAL;
    spg_ctx *c = new spg_ctx;
    c->be = *backend;
    c->is_hip = false;
    *out = c;
    return 0;
}

extern "C" int spg_get_unique_id(void *id_out) {
    if (!id_out) return SPG_EINVAL;
    char err[256];
    int rc = spg::rccl_get_unique_id(id_out, err, sizeof err);
    if (rc) fprintf(stderr, "libspg_hip: %s\n", err);
    return rc;
}

extern "C" int spg_ctx_create_ranks(spg_ctx **out, int device, int rank, int nranks, const void *nccl_unique_id) {
    if (!out || nranks < 1 || rank < 0 || rank >= nranks) return SPG_EINVAL;
    int rc = spg_ctx_create(out, device);
    if (rc) return rc;
    spg_ctx *c = *out;
    c->rank = rank; c->nranks = nranks;
    if (nccl_unique_id) {
        rc = spg::rccl_comm_create(device, rank, nranks, nccl_unique_id, &c->rccl, c->err, sizeof c->err);
        if (rc) {
            fprintf(stderr, "libspg_hip: %s\n", c->err);
            spg_ctx_destroy(c);
            *out = nullptr;
            return rc;
        }
    }
    return 0;
}
extern "C" int spg_ctx_set_linear_solver(spg_ctx *c, int solver) {
    if (!c || solver < SPG_SOLVER_AUTO || solver > SPG_SOLVER_PCG) return SPG_EINVAL;
    c->linear_solver = solver;
    return 0;
}
extern "C" int spg_ctx_set_pcg(spg_ctx *c, double rel_tol, int max_iter) {
    if (!c || std::isnan(rel_tol)) return SPG_EINVAL;
    c->pcg_rel_tol = rel_tol > 0 ? rel_tol : 0;
    c->pcg_max_iter = max_iter > 0 ? max_iter : 0;
    return 0;
}
extern "C" int spg_ctx_set_factor_descent(spg_ctx *c, double rel_tol, int max_cycles) {
    if (!c || std::isnan(rel_tol) || max_cycles > 32767) return SPG_EINVAL;
    // rel_tol == 0 with a cycle count: exactly that many cycles; otherwise a value <= 0 selects the default
    const int cycles = max_cycles > 0 ? max_cycles : spg::kFdMaxCycles;
    const double tol = rel_tol > 0 ? rel_tol : (rel_tol == 0 && max_cycles > 0) ? 0.0 : spg::kFdRelTol;
    if (c->is_hip) spg::hip_backend_set_factor_descent(&c->be, tol, cycles);    // (other backends ignore the flag)
    return 0;
}
extern "C" int spg_ctx_pcg_stats(spg_ctx *c, spg_pcg_stats *out) {
    if (!c || !out) return SPG_EINVAL;
    *out = c->pcg_stats;
    return 0;
}
extern "C" int spg_ctx_set_greedy_method(spg_ctx *c, int method, int lookahead) {
    if (!c || method < SPG_GREEDY_JOINT || method > SPG_GREEDY_AUTO || lookahead < 0) return SPG_EINVAL;
    c->greedy_method = method;
    c->greedy_lookahead = lookahead;
    return 0;
}
extern "C" int spg_ctx_greedy_stats(spg_ctx *c, spg_greedy_stats *out) {
    if (!c || !out) return SPG_EINVAL;
    *out = c->greedy_stats;
    return 0;
}

extern "C" int spg_ctx_rank(const spg_ctx *c) { return c ? c->rank : 0; }
extern "C" int spg_ctx_nranks(const spg_ctx *c) { return c ? c->nranks : 0; }

extern "C" int spg_allgather_region(spg_ctx *c, void *arena, int64_t region_off, int64_t chunk_len) {
    if (!c || !arena || region_off < 0 || chunk_len < 0) return SPG_EINVAL;
    if (!c->rccl) {
        // a multi-rank context without a communicator cannot exchange: committing un-gathered chunks would silently
        // diverge the replicas (single-rank contexts: nothing to do)
        if (c->nranks > 1) return set_err(c, SPG_ESTATE, "spg_allgather_region: the context has %s ranks but no RCCL communicator (spg_ctx_create_ranks without a unique id)", std::to_string(c->nranks).c_str());
        return 0;
    }
    return spg::rccl_allgather_f64(c->rccl, arena, region_off, chunk_len, spg::hip_backend_stream(&c->be), c->err, sizeof c->err);
}

extern "C" void spg_ctx_destroy(spg_ctx *c) {
    if (!c) return;
    if (c->rccl) spg::rccl_comm_destroy(c->rccl);
    if (c->is_hip) spg::hip_backend_destroy(&c->be);
    delete c;
}
extern "C" void spg_free(void *p) { free(p); }

extern "C" const char *spg_last_error(spg_ctx *c) {
    if (!c) return "";
    if (c->err[0]) return c->err;
    return c->is_hip ? spg::hip_backend_error(&c->be) : "";
}
extern "C" void *spg_ctx_stream(spg_ctx *c) { return (c && c->is_hip) ? spg::hip_backend_stream(&c->be) : nullptr; }
extern "C" int spg_ctx_synchronize(spg_ctx *c) { return c ? c->be.synchronize(c->be.user) : SPG_EINVAL; }

extern "C" int spg_ctx_profile(spg_ctx *c, int enable) {
    if (!c || !c->is_hip) return SPG_EINVAL;
    spg::hip_backend_profile(&c->be, enable);
    return 0;
}
extern "C" int spg_ctx_profile_read_worker(spg_ctx *c, double *kernel_ms, double *alg_bytes, int64_t *runs, int64_t *blankets) {
    if (!c || !c->is_hip || !kernel_ms || !alg_bytes || !runs || !blankets) return SPG_EINVAL;
    long long r = 0, b = 0;
    spg::hip_backend_profile_read_worker(&c->be, kernel_ms, alg_bytes, &r, &b);
    *runs = r; *blankets = b;
    return 0;
}
extern "C" int spg_ctx_profile_read_big(spg_ctx *c, double *kernel_ms, double *flops, int64_t *blankets, int32_t *n_max) {
    if (!c || !c->is_hip || !kernel_ms || !flops || !blankets || !n_max) return SPG_EINVAL;
    long long cnt = 0;
    int nm = 0;
    spg::hip_backend_profile_read_big(&c->be, kernel_ms, flops, &cnt, &nm);
    *blankets = cnt; *n_max = nm;
    return 0;
}
extern "C" int spg_ctx_profile_read(spg_ctx *c, double *kernel_ms, double *alg_bytes, int64_t *launches, int64_t *blankets) {
    if (!c || !c->is_hip || !kernel_ms || !alg_bytes || !launches || !blankets) return SPG_EINVAL;
    long long l = 0, b = 0;
    spg::hip_backend_profile_read(&c->be, kernel_ms, alg_bytes, &l, &b);
    *launches = l; *blankets = b;
    return 0;
}

// ================================================================================= decimation
// src/decimation.cpp:11-49
static int emit(const std::vector<int> &v, int32_t *out, int cap) {
    for (size_t i = 0; i < v.size() && (int)i < cap; i++) out[i] = v[i];
    return (int)v.size();
}
extern "C" int spg_decimate_cluster(int last, int endvert, int sparsity, int clusterSize, int32_t *out, int cap) {
    std::vector<int> ret;
    if (clusterSize > 0 && (((last - 4) % clusterSize == 0 && last > 4) || last == endvert)) {
        for (int i = int(std::ceil((last - 5) / (double)clusterSize) - 1) * clusterSize + 5; i <= last; i++)
            if (i % sparsity > 0) ret.push_back(i);
    }
    return emit(ret, out, cap);
}
extern "C" int spg_decimate_online(int last, int, int sparsity, int, int32_t *out, int cap) {
    std::vector<int> ret;
    if (last % sparsity != 0) ret.push_back(last);
    return emit(ret, out, cap);
}
extern "C" int spg_decimate_global(int last, int endvert, int sparsity, int, int32_t *out, int cap) {
    std::vector<int> ret;
    if (last == endvert)
        for (int i = 4; i <= endvert; i++)
            if (i % sparsity != 0) ret.push_back(i);
    return emit(ret, out, cap);
}

// ================================================================================= arena
int sync_host(spg_graph *g) {  // pull device-only ranges into the host mirror
    if (g->stale_hi > g->stale_lo) {
        if ((int64_t)g->host.size() < g->used) g->host.resize((size_t)g->used);
        int rc = g->ctx->be.download(g->ctx->be.user, g->host.data() + g->stale_lo,
                                     (char *)g->dev + g->stale_lo * 8, g->stale_hi - g->stale_lo);
        if (rc) return rc;
        g->stale_lo = g->stale_hi = 0;
    }
    return 0;
}

int sync_device(spg_graph *g) {  // push host-only tail to the device
    if (g->dev_synced < g->used) {
        if (int rc = arena_ensure(g, g->used)) return rc;
        int64_t lo = g->dev_synced;
        // the tail may overlap a stale (device-only) range only if it was produced on the device,
        // in which case dev_synced already covers it
        int rc = g->ctx->be.upload(g->ctx->be.user, (char *)g->dev + lo * 8, g->host.data() + lo, g->used - lo);
        if (rc) return rc;
        g->dev_synced = g->used;
    }
    return 0;
}

int arena_ensure(spg_graph *g, int64_t need) {
    if (need <= g->cap && g->dev) return 0;
    if (int rc = sync_host(g)) return rc;
    int64_t nc = std::max<int64_t>(need, std::max<int64_t>(g->cap * 2, 1 << 16));
    void *nd = g->ctx->be.alloc(g->ctx->be.user, nc);
    if (!nd) return set_err(g->ctx, SPG_ENOMEM, "arena allocation failed");
    if (g->dev) g->ctx->be.release(g->ctx->be.user, g->dev);
    g->dev = nd;
    g->cap = nc;
    g->dev_synced = 0;
    if ((int64_t)g->host.size() < g->used) g->host.resize((size_t)g->used);
    return 0;
}

static int64_t arena_push(spg_graph *g, const double *src, int64_t len) {
    int64_t off = g->used;
    if ((int64_t)g->host.size() < off + len) g->host.resize((size_t)std::max<int64_t>(off + len, (int64_t)g->host.size() * 2));
    if (src) memcpy(g->host.data() + off, src, (size_t)len * 8);
    g->used += len;
    return off;
}

// ================================================================================= graph basics
extern "C" int spg_graph_create(spg_ctx *ctx, int pose_dim, spg_graph **out) {
    if (!ctx || !out || (pose_dim != 3 && pose_dim != 6)) return SPG_EINVAL;
    spg_graph *g = new spg_graph;
    g->ctx = ctx;
    g->d = pose_dim;
    g->ps = pose_stride(pose_dim);
    g->rec = g->ps + info_len(pose_dim);
    *out = g;
    return 0;
}

extern "C" void spg_graph_destroy(spg_graph *g) {
    if (!g) return;
    if (g->dev) g->ctx->be.release(g->ctx->be.user, g->dev);
    delete g;
}

extern "C" int spg_graph_add_vertex(spg_graph *g, int id, const double *pose) {
    if (!g || !pose || g->active) return SPG_EINVAL;
    if (g->vidx.count(id)) return set_err(g->ctx, SPG_EINVAL, "duplicate vertex id");
    int32_t idx = (int32_t)g->vid.size();
    g->vid.push_back(id);
    g->vidx[id] = idx;
    if (g->vdirect_ok) {
        if (id < 0 || (size_t)id > 8 * g->vid.size() + 4096) { g->vdirect_ok = false; g->vdirect.clear(); g->vdirect.shrink_to_fit(); }
        else { if ((size_t)id >= g->vdirect.size()) g->vdirect.resize(std::max<size_t>((size_t)id + 1, g->vdirect.size() * 2), -1); g->vdirect[(size_t)id] = idx; }
    }
    g->valive.push_back(1);
    g->vr.emplace_back();
    g->vown.emplace_back();
    g->vpose.push_back(arena_push(g, pose, g->ps));
    g->vr.back().id = id;
    g->vr.back().pose = g->vpose.back();
    g->n_live_v++;
    return 0;
}

int add_edge_idx(spg_graph *g, int kind, int nv, const int32_t *vix, int64_t off, int32_t len, int64_t key) {
    // the submission thread reads edges[] / everts[] of batches in its queue: never move them under it
    if (g->sub_active && (g->edges.size() == g->edges.capacity() || (nv != 2 && g->everts.size() + (size_t)nv > g->everts.capacity()))) {
        quiesce_submission(g);
        g->edges.reserve(std::max<size_t>(g->edges.capacity() * 2, 1024));
        g->everts.reserve(std::max<size_t>(g->everts.capacity() * 2 + (size_t)nv, 1024));
    }
    GEdge e;
    e.kind = (int8_t)kind; e.nv = (int16_t)nv; e.len = len; e.off = off; e.alive = 1;
    e.key = key >= 0 ? key : g->next_key++;
    if (nv == 2) { e.vtx[0] = vix[0]; e.vtx[1] = vix[1]; }
    else { e.vtx[0] = (int32_t)g->everts.size(); e.vtx[1] = 0; }
    int32_t eid = (int32_t)g->edges.size();
    if (nv != 2) for (int i = 0; i < nv; i++) g->everts.push_back(vix[i]);
    g->edges.push_back(e);
    g->n_mutations++;
    for (int i = 0; i < nv; i++) {
        bool dup = false;
        for (int j = 0; j < i; j++) dup |= (vix[j] == vix[i]);
        if (!dup) g->vr[vix[i]].adj.push_back({eid, (nv == 2 && kind == SPG_EDGE_BINARY) ? vix[1 - i] : -1});
    }
    g->n_live_e++;
    return eid;
}

extern "C" int spg_graph_add_edge(spg_graph *g, int from, int to, const double *meas, const double *info_upper) {
    if (!g || !meas || !info_upper || g->active) return SPG_EINVAL;
    auto a = g->vidx.find(from), b = g->vidx.find(to);
    if (a == g->vidx.end() || b == g->vidx.end() || !g->valive[a->second] || !g->valive[b->second])
        return set_err(g->ctx, SPG_EINVAL, "edge endpoint does not exist");
    int64_t off = arena_push(g, meas, g->ps);
    arena_push(g, info_upper, info_len(g->d));
    int32_t vix[2] = {a->second, b->second};
    add_edge_idx(g, SPG_EDGE_BINARY, 2, vix, off, g->rec);
    return 0;
}

extern "C" int spg_graph_add_glc_edge(spg_graph *g, int q, const int32_t *ids, int r, const double *meas, const double *W) {
    if (!g || q < 1 || r < 1 || !ids || !meas || !W || g->active) return SPG_EINVAL;
    std::vector<int32_t> vix(q);
    for (int i = 0; i < q; i++) {
        auto it = g->vidx.find(ids[i]);
        if (it == g->vidx.end() || !g->valive[it->second]) return set_err(g->ctx, SPG_EINVAL, "edge endpoint does not exist");
        vix[i] = it->second;
    }
    int n = g->d * q;
    int64_t off = arena_push(g, meas, n);
    arena_push(g, W, (int64_t)r * n);
    add_edge_idx(g, SPG_EDGE_GLC, q, vix.data(), off, n + r * n);
    return 0;
}

extern "C" int spg_graph_add_multi_edge(spg_graph *g, int q, const int32_t *ids, const double *record, int64_t len) {
    if (!g || q < 2 || !ids || !record || g->active) return SPG_EINVAL;
    const int nm = (int)record[0];
    if (nm < 1 || len != SPG_MULTI_LEN(g->d, nm)) return set_err(g->ctx, SPG_EINVAL, "multi edge record length does not match its measurement count");
    for (int i = 0; i < 2 * nm; i++) if (record[1 + i] < 0 || record[1 + i] >= q) return set_err(g->ctx, SPG_EINVAL, "multi edge: a measurement refers to a vertex outside the edge");
    std::vector<int32_t> vix(q);
    for (int i = 0; i < q; i++) {
        auto it = g->vidx.find(ids[i]);
        if (it == g->vidx.end() || !g->valive[it->second]) return set_err(g->ctx, SPG_EINVAL, "edge endpoint does not exist");
        vix[i] = it->second;
    }
    int64_t off = arena_push(g, record, len);
    add_edge_idx(g, SPG_EDGE_MULTI, q, vix.data(), off, (int32_t)len);
    return 0;
}

// bulk forms of addVertex / addEdge (same semantics, one call per array)
extern "C" int spg_graph_add_vertices(spg_graph *g, int n, const int32_t *ids, const double *poses) {
    if (!g || n < 0 || !ids || !poses) return SPG_EINVAL;
    g->vid.reserve(g->vid.size() + n);
    for (int i = 0; i < n; i++)
        if (int rc = spg_graph_add_vertex(g, ids[i], poses + (size_t)i * g->ps)) return rc;
    return 0;
}
extern "C" int spg_graph_add_edges(spg_graph *g, int n, const int32_t *ij, const double *records) {
    if (!g || n < 0 || !ij || !records) return SPG_EINVAL;
    g->edges.reserve(g->edges.size() + n);
    for (int i = 0; i < n; i++) {
        const double *r = records + (size_t)i * g->rec;
        if (int rc = spg_graph_add_edge(g, ij[2 * i], ij[2 * i + 1], r, r + g->ps)) return rc;
    }
    return 0;
}

extern "C" int spg_graph_pose_dim(const spg_graph *g) { return g ? g->d : 0; }
extern "C" int spg_graph_num_vertices(const spg_graph *g) { return g ? g->n_live_v : 0; }
extern "C" int spg_graph_num_edges(const spg_graph *g) { return g ? g->n_live_e : 0; }
// The streaming driver appends new edges in the order their blankets happen to complete, which varies from run to run.
// Results never depend on it (blanket edges are summed in key order), but everything that EXPOSES the edge array's order
// does: spg_graph_get_edges / the .g2o writer / clones, and the dense assembly, which sums a vertex's incident edges in
// array order. Before any of those the tail the stream appended is put into key order — the order the sequential loop
// would have inserted the edges in — so that two runs on the same input hand out byte-identical graphs. Lazy: it costs
// ~3 ms on the 100k-pose graph and a marginalisation that is only followed by another one never pays it.
void canonicalize_edge_order(spg_graph *g) {
    if (g->unsorted_from < 0 || g->active) return;
    const size_t from = (size_t)g->unsorted_from, n = g->edges.size() - from;
    g->unsorted_from = -1;
    if (n < 2) return;
    std::vector<uint32_t> perm(n);
    for (size_t i = 0; i < n; i++) perm[i] = (uint32_t)i;
    bool sorted = true;
    for (size_t i = 1; i < n && sorted; i++) sorted = g->edges[from + i - 1].key <= g->edges[from + i].key;
    if (sorted) return;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return g->edges[from + a].key < g->edges[from + b].key; });
    std::vector<int32_t> newid(n);
    std::vector<GEdge> tmp(n);
    for (size_t i = 0; i < n; i++) { tmp[i] = g->edges[from + perm[i]]; newid[perm[i]] = (int32_t)(from + i); }
    std::copy(tmp.begin(), tmp.end(), g->edges.begin() + (long)from);
    next_stamp(g);
    const int32_t st = g->stamp;
    for (size_t i = 0; i < n; i++) {
        const GEdge &e = g->edges[from + i];
        if (!e.alive) continue;
        for (int t = 0; t < e.nv; t++) {
            const int32_t v = edge_verts(g, e)[t];
            if (g->vstamp[v] == st) continue;
            g->vstamp[v] = st;
            for (auto &a : g->vr[v].adj) if ((size_t)a.eid >= from) a.eid = newid[(size_t)a.eid - from];
        }
    }
    g->n_mutations++;
}

extern "C" int64_t spg_graph_edge_data_size(const spg_graph *g) {
    int64_t s = 0;
    for (auto &e : g->edges) if (e.alive) s += e.len;
    return s;
}
extern "C" int64_t spg_graph_edge_vert_size(const spg_graph *g) {
    int64_t s = 0;
    for (auto &e : g->edges) if (e.alive) s += e.nv;
    return s;
}

extern "C" int spg_graph_get_vertices(spg_graph *g, int32_t *ids, double *poses) {
    if (!g) return SPG_EINVAL;
    if (int rc = sync_host(g)) return rc;
    std::vector<std::pair<int32_t, int32_t>> order;
    for (size_t i = 0; i < g->vid.size(); i++) if (g->valive[i]) order.push_back({g->vid[i], (int32_t)i});
    std::sort(order.begin(), order.end());
    for (size_t k = 0; k < order.size(); k++) {
        ids[k] = order[k].first;
        memcpy(poses + k * g->ps, g->host.data() + g->vpose[order[k].second], (size_t)g->ps * 8);
    }
    return (int)order.size();
}

extern "C" int spg_graph_get_edges(spg_graph *g, int32_t *kind, int32_t *vert_off, int32_t *vert_ids, int64_t *data_off, double *data) {
    if (!g) return SPG_EINVAL;
    canonicalize_edge_order(g);
    if (int rc = sync_host(g)) return rc;
    int ne = 0, nv = 0;
    int64_t nd = 0;
    vert_off[0] = 0; data_off[0] = 0;
    for (auto &e : g->edges) {
        if (!e.alive) continue;
        kind[ne] = e.kind;
        for (int i = 0; i < e.nv; i++) vert_ids[nv++] = g->vid[edge_verts(g, e)[i]];
        memcpy(data + nd, g->host.data() + e.off, (size_t)e.len * 8);
        nd += e.len;
        ne++;
        vert_off[ne] = nv; data_off[ne] = nd;
    }
    return ne;
}

extern "C" int spg_graph_remove_edges(spg_graph *g, const int32_t *edge_idx, int n) {
    const char *what = "spg_graph_remove_edges";
    if (!g || n < 0 || (n > 0 && !edge_idx)) return SPG_EINVAL;
    if (g->active) return set_err(g->ctx, SPG_EINVAL, "%s: a stepwise marginalisation is active", what);
    canonicalize_edge_order(g);
    std::vector<int32_t> live;
    live.reserve((size_t)g->n_live_e);
    for (size_t e = 0; e < g->edges.size(); e++) if (g->edges[e].alive) live.push_back((int32_t)e);
    std::unordered_set<int32_t> seen;
    for (int i = 0; i < n; i++) {
        const int32_t x = edge_idx[i];
        const char *why = (x < 0 || (size_t)x >= live.size()) ? "is out of range" : !seen.insert(x).second ? "is listed twice" : nullptr;
        if (why) {
            snprintf(g->ctx->err, sizeof g->ctx->err, "%s: entry %d: edge %d %s", what, i, (int)x, why);
            return SPG_EINVAL;
        }
    }
    for (int i = 0; i < n; i++) retire_edge(g, live[edge_idx[i]]);
    return 0;
}

extern "C" int spg_graph_set_estimate(spg_graph *g, int id, const double *pose) {
    if (!g || !pose || g->active) return SPG_EINVAL;
    auto it = g->vidx.find(id);
    if (it == g->vidx.end() || !g->valive[it->second]) return SPG_EINVAL;
    int64_t off = g->vpose[it->second];
    memcpy(g->host.data() + off, pose, (size_t)g->ps * 8);
    if (off < g->dev_synced && g->dev)
        return g->ctx->be.upload(g->ctx->be.user, (char *)g->dev + off * 8, pose, g->ps);
    return 0;
}

extern "C" void *spg_graph_arena(spg_graph *g, int64_t *capacity) {
    if (!g) return nullptr;
    if (capacity) *capacity = g->cap;
    return g->dev;
}

extern "C" int spg_graph_reserve(spg_graph *g, int64_t arena_doubles) {
    if (!g) return SPG_EINVAL;
    if (int rc = arena_ensure(g, std::max(arena_doubles, g->used))) return rc;
    // The host mirror is reserved AND touched up to the same size: the commit copies every batch's out records into it,
    // and a first touch there is a page fault inside the timed path — with transparent huge pages a 2 MB zero-fill
    // (~100 us) per fault, ~150 of them per 100 k-pose marginalisation on the mirrors the kernel happened to back with
    // huge pages (measured: 25 ms per call on some graphs, 55 ms on others, device time identical).
    if ((int64_t)g->host.size() < g->cap) g->host.resize((size_t)g->cap);
    // the same for the containers a marginalisation appends to: room for as many new edges as there are now, touched
    {
        const size_t ne = g->edges.size(), nl = g->log.size();
        g->edges.resize(2 * ne + 1024); g->edges.resize(ne);
        g->log.resize(g->vid.size() + 16); g->log.resize(nl);
        // and the scheduler's own scratch, to the sizes a few hundred blankets per batch need (they grow past that as ever)
        auto touch = [](auto &v, size_t n) { if (v.capacity() < n) { const size_t keep = v.size(); v.resize(n); v.resize(keep); } };
        const size_t nv = g->vid.size();
        for (int i = 0; i < spg_graph::NB; i++) {
            Batch &b = g->bt[i];
            touch(b.rb, 1024); touch(b.rb_verts, 16384); touch(b.rb_edges, 32768); touch(b.h_blk, 1024); touch(b.h_vpo, 16384);
            touch(b.h_er, 32768); touch(b.h_ev, 65536); touch(b.kld_pending, 1024);
        }
        touch(g->pending, nv); touch(g->in_set, nv); touch(g->vstamp, nv); touch(g->estamp, 2 * ne + 1024);
        touch(g->owners, 8192); touch(g->ocnt, 8192); touch(g->owner_free, 8192); touch(g->transient, 4096); touch(g->Dpool, 65536);
        touch(g->s_newpending, 4096); touch(g->hdr_buf, 65536);
    }
    return sync_device(g);
}

// ================================================================================= .g2o I/O
static void normalize_quat(double *q) {
    double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (n > 0) for (int i = 0; i < 4; i++) q[i] /= n;
}

extern "C" int spg_graph_load_g2o(spg_ctx *ctx, const char *path, spg_graph **out) {
    if (!ctx || !path || !out) return SPG_EINVAL;
    FILE *f = fopen(path, "r");
    if (!f) return set_err(ctx, SPG_EIO, "cannot open %s", path);
    struct V { int id; double p[7]; };
    struct E { int a, b; double r[28]; };
    struct GE { std::vector<int32_t> ids; int r = 0, n = 0; std::vector<double> meas, W; };
    std::vector<V> vs;
    std::vector<E> es;
    std::vector<GE> ges;
    int d = 0;
    char *lbuf = nullptr;   // getline: a Dense GLC edge is one line of r*n numbers, far beyond any fixed buffer
    size_t lcap = 0;
    bool bad_glc = false, has_multi = false;
    while (getline(&lbuf, &lcap, f) >= 0) {
        char *s = lbuf;
        while (*s == ' ' || *s == '\t') s++;
        char tag[64];
        int adv = 0;
        if (sscanf(s, "%63s%n", tag, &adv) != 1) continue;
        s += adv;
        auto readn = [&](double *dst, int cnt) {
            for (int i = 0; i < cnt; i++) {
                char *end;
                dst[i] = strtod(s, &end);
                if (end == s) return false;
                s = end;
            }
            return true;
        };
        auto readi = [&](int &v) {
            char *end;
            long x = strtol(s, &end, 10);
            if (end == s) return false;
            v = (int)x; s = end;
            return true;
        };
        if (!strcmp(tag, "VERTEX_SE2")) {
            V v{};
            if (!readi(v.id) || !readn(v.p, 3)) continue;
            if (!d) d = 3;
            vs.push_back(v);
        } else if (!strcmp(tag, "VERTEX_SE3:QUAT")) {
            V v{};
            if (!readi(v.id) || !readn(v.p, 7)) continue;
            normalize_quat(v.p + 3);
            if (!d) d = 6;
            vs.push_back(v);
        } else if (!strcmp(tag, "EDGE_SE2")) {
            E e{};
            if (!readi(e.a) || !readi(e.b) || !readn(e.r, 9)) continue;
            es.push_back(e);
        } else if (!strcmp(tag, "EDGE_SE3:QUAT")) {
            E e{};
            if (!readi(e.a) || !readi(e.b) || !readn(e.r, 28)) continue;
            normalize_quat(e.r + 3);
            es.push_back(e);
        } else if (!strcmp(tag, "GLC_EDGE")) {
            // GLCEdge::read (src/glc_edge.cpp:65-93) behind g2o's hyper-edge prefix "id id ... ||":
            // <reparam tag> r n, measurement (n), W (r x n, row-major), information (upper triangle, r x r)
            GE ge;
            for (;;) {
                while (*s == ' ' || *s == '\t') s++;
                if (s[0] == '|' && s[1] == '|') { s += 2; break; }
                int id;
                if (!readi(id)) { bad_glc = true; break; }
                ge.ids.push_back(id);
            }
            char rtag[64];
            int adv2 = 0;
            if (bad_glc || sscanf(s, "%63s%n", rtag, &adv2) != 1) { bad_glc = true; continue; }
            s += adv2;
            if (!readi(ge.r) || !readi(ge.n) || ge.r < 1 || ge.n < 1 || ge.ids.empty() || ge.n % (int)ge.ids.size()) { bad_glc = true; continue; }
            ge.meas.resize(ge.n);
            ge.W.resize((size_t)ge.r * ge.n);
            std::vector<double> info((size_t)ge.r * (ge.r + 1) / 2);
            if (!readn(ge.meas.data(), ge.n) || !readn(ge.W.data(), ge.r * ge.n) || !readn(info.data(), (int)info.size())) { bad_glc = true; continue; }
            // the reference writes information = I_r; a general SPD information is folded into W (W <- L^T W, Omega = L L^T)
            bool ident = true;
            {
                size_t p2 = 0;
                for (int i = 0; i < ge.r; i++) for (int j = i; j < ge.r; j++) { ident &= (info[p2] == (i == j ? 1.0 : 0.0)); p2++; }
            }
            if (!ident) {
                std::vector<double> Lm((size_t)ge.r * ge.r, 0.0);
                size_t p2 = 0;
                for (int i = 0; i < ge.r; i++) for (int j = i; j < ge.r; j++) { Lm[(size_t)j * ge.r + i] = info[p2]; p2++; }   // lower triangle
                bool pd = true;
                for (int j = 0; j < ge.r && pd; j++) {
                    double dj = Lm[(size_t)j * ge.r + j];
                    for (int k = 0; k < j; k++) dj -= Lm[(size_t)j * ge.r + k] * Lm[(size_t)j * ge.r + k];
                    if (!(dj > 0)) { pd = false; break; }
                    double l = std::sqrt(dj);
                    Lm[(size_t)j * ge.r + j] = l;
                    for (int i = j + 1; i < ge.r; i++) {
                        double sacc = Lm[(size_t)i * ge.r + j];
                        for (int k = 0; k < j; k++) sacc -= Lm[(size_t)i * ge.r + k] * Lm[(size_t)j * ge.r + k];
                        Lm[(size_t)i * ge.r + j] = sacc / l;
                    }
                }
                if (!pd) { bad_glc = true; continue; }
                std::vector<double> W2((size_t)ge.r * ge.n, 0.0);
                for (int i = 0; i < ge.r; i++) for (int k = i; k < ge.r; k++) for (int c = 0; c < ge.n; c++) W2[(size_t)i * ge.n + c] += Lm[(size_t)k * ge.r + i] * ge.W[(size_t)k * ge.n + c];
                ge.W.swap(W2);
            }
            ges.push_back(std::move(ge));
        } else if (!strncmp(tag, "MULTI_EDGE_", 11)) {
            // MultiEdgeCorrelated::write (src/multi_edge_correlated.hpp:227-267) does not say which vertex pair each
            // measurement belongs to — the reference's own read() cannot restore the edge either. Dropping the line would
            // hand back a graph without its correlated constraints (possibly disconnected) and no error: refuse the file.
            has_multi = true;
        }
    }
    free(lbuf);
    fclose(f);
    if (has_multi) return set_err(ctx, SPG_EIO, "%s holds MULTI_EDGE_* records: that format omits the vertex pair of each measurement and cannot be read back", path);
    if (bad_glc) return set_err(ctx, SPG_EIO, "malformed GLC_EDGE record in %s", path);
    if (!d) return set_err(ctx, SPG_EIO, "no SE2/SE3 vertices in %s", path);
    std::stable_sort(vs.begin(), vs.end(), [](const V &a, const V &b) { return a.id < b.id; });
    spg_graph *g;
    if (int rc = spg_graph_create(ctx, d, &g)) return rc;
    for (auto &v : vs) if (int rc = spg_graph_add_vertex(g, v.id, v.p)) { spg_graph_destroy(g); return rc; }
    for (auto &e : es) if (int rc = spg_graph_add_edge(g, e.a, e.b, e.r, e.r + g->ps)) { spg_graph_destroy(g); return rc; }
    for (auto &ge : ges) {
        if (ge.n != d * (int)ge.ids.size()) { spg_graph_destroy(g); return set_err(ctx, SPG_EIO, "GLC_EDGE dimension does not match its vertices in %s", path); }
        if (int rc = spg_graph_add_glc_edge(g, (int)ge.ids.size(), ge.ids.data(), ge.r, ge.meas.data(), ge.W.data())) { spg_graph_destroy(g); return rc; }
    }
    *out = g;
    return 0;
}

static void write_g2o_stream(spg_graph *g, FILE *f);
extern "C" int spg_graph_write_g2o(spg_graph *g, const char *path) {
    if (!g || !path) return SPG_EINVAL;
    if (int rc = sync_host(g)) return rc;
    FILE *f = fopen(path, "w");
    if (!f) return set_err(g->ctx, SPG_EIO, "cannot open %s for writing", path);
    write_g2o_stream(g, f);
    fclose(f);
    return 0;
}
extern "C" int spg_graph_write_g2o_mem(spg_graph *g, char **text, size_t *len) {
    if (!g || !text || !len) return SPG_EINVAL;
    if (int rc = sync_host(g)) return rc;
    *text = nullptr; *len = 0;
    FILE *f = open_memstream(text, len);
    if (!f) return set_err(g->ctx, SPG_ENOMEM, "open_memstream failed");
    write_g2o_stream(g, f);
    fclose(f);   // finalises *text / *len (NUL-terminated)
    return 0;
}
static void write_g2o_stream(spg_graph *g, FILE *f) {
    canonicalize_edge_order(g);
    std::vector<std::pair<int32_t, int32_t>> order;
    for (size_t i = 0; i < g->vid.size(); i++) if (g->valive[i]) order.push_back({g->vid[i], (int32_t)i});
    std::sort(order.begin(), order.end());
    const char *vt = g->d == 3 ? "VERTEX_SE2" : "VERTEX_SE3:QUAT", *et = g->d == 3 ? "EDGE_SE2" : "EDGE_SE3:QUAT";
    for (auto &o : order) {
        fprintf(f, "%s %d", vt, o.first);
        for (int i = 0; i < g->ps; i++) fprintf(f, " %.17g", g->host[g->vpose[o.second] + i]);
        fputc('\n', f);
    }
    for (auto &e : g->edges) {
        if (!e.alive) continue;
        if (e.kind == SPG_EDGE_BINARY) {
            fprintf(f, "%s %d %d", et, g->vid[edge_verts(g, e)[0]], g->vid[edge_verts(g, e)[1]]);
            for (int i = 0; i < e.len; i++) fprintf(f, " %.17g", g->host[e.off + i]);
        } else if (e.kind == SPG_EDGE_MULTI) {
            // MultiEdgeCorrelated::write (src/multi_edge_correlated.hpp:227-267): "|| nmeas nrelevant meas... info(upper)". As in
            // the reference the vertex pair of each measurement is NOT part of the line (its own reader cannot restore it).
            const double *rec = g->host.data() + e.off;
            const int nm = (int)rec[0], r = g->d * nm;
            const double *meas = rec + 1 + 2 * nm, *W = meas + (size_t)nm * g->ps;
            fprintf(f, "%s", g->d == 3 ? "MULTI_EDGE_SE2" : "MULTI_EDGE_SE3");
            for (int i = 0; i < e.nv; i++) fprintf(f, " %d", g->vid[edge_verts(g, e)[i]]);
            fprintf(f, " || %d %d", nm, g->ps);
            for (int i = 0; i < nm * g->ps; i++) fprintf(f, " %.17g", meas[i]);
            for (int i = 0; i < r; i++) for (int j = i; j < r; j++) {
                double v = 0;
                for (int t = 0; t < r; t++) v += W[(size_t)t * r + i] * W[(size_t)t * r + j];
                fprintf(f, " %.17g", v);
            }
        } else {
            // GLCEdge::write (src/glc_edge.cpp:95-119): "|| <reparam tag> r dq meas W info(upper of I_r)"
            int n = g->d * e.nv, r = (e.len - n) / n;
            fprintf(f, "GLC_EDGE");
            for (int i = 0; i < e.nv; i++) fprintf(f, " %d", g->vid[edge_verts(g, e)[i]]);
            fprintf(f, " || %s %d %d", g->d == 3 ? "GLC_REPARAM_SE2_ISAM" : "GLC_REPARAM_SE3", r, n);
            for (int i = 0; i < e.len; i++) fprintf(f, " %.17g", g->host[e.off + i]);
            for (int i = 0; i < r; i++) for (int j = i; j < r; j++) fprintf(f, " %d", i == j ? 1 : 0);
        }
        fputc('\n', f);
    }
}

// GraphWrapperG2O::clonePortion (src/graph_wrapper_g2o.cpp:334-356)
extern "C" int spg_graph_clone_portion(spg_graph *g, int maxid, spg_graph **out) {
    if (!g || !out || g->active) return SPG_EINVAL;
    canonicalize_edge_order(g);
    if (int rc = sync_host(g)) return rc;
    spg_graph *c;
    if (int rc = spg_graph_create(g->ctx, g->d, &c)) return rc;
    std::vector<std::pair<int32_t, int32_t>> order;
    for (size_t i = 0; i < g->vid.size(); i++) if (g->valive[i] && g->vid[i] <= maxid) order.push_back({g->vid[i], (int32_t)i});
    std::sort(order.begin(), order.end());
    int rc = 0;
    for (auto &o : order) if ((rc = spg_graph_add_vertex(c, o.first, g->host.data() + g->vpose[o.second]))) break;
    std::vector<int32_t> ids;
    for (size_t ei = 0; ei < g->edges.size() && !rc; ei++) {
        const GEdge &e = g->edges[ei];
        if (!e.alive) continue;
        bool in = true;
        ids.clear();
        for (int i = 0; i < e.nv; i++) { int32_t id = g->vid[edge_verts(g, e)[i]]; in &= (id <= maxid); ids.push_back(id); }
        if (!in) continue;
        const double *rec = g->host.data() + e.off;
        if (e.kind == SPG_EDGE_BINARY) rc = spg_graph_add_edge(c, ids[0], ids[1], rec, rec + g->ps);
        else if (e.kind == SPG_EDGE_MULTI) rc = spg_graph_add_multi_edge(c, e.nv, ids.data(), rec, e.len);
        else { int n = g->d * e.nv; rc = spg_graph_add_glc_edge(c, e.nv, ids.data(), (e.len - n) / n, rec, rec + n); }
    }
    if (rc) { spg_graph_destroy(c); return rc; }
    c->robust_kind = g->robust_kind; c->robust_delta = g->robust_delta; c->robust_gap = g->robust_gap;
    *out = c;
    return 0;
}

// GraphWrapper::Vertex::edges() (src/graph_wrapper.h:26)
extern "C" int spg_graph_vertex_edges(spg_graph *g, int id, int32_t *edge_index, int cap) {
    if (!g || (cap > 0 && !edge_index)) return SPG_EINVAL;
    auto it = g->vidx.find(id);
    if (it == g->vidx.end() || !g->valive[it->second]) return set_err(g->ctx, SPG_EINVAL, "no such vertex");
    std::vector<int32_t> es(g->vr[it->second].adj.begin(), g->vr[it->second].adj.end());
    std::sort(es.begin(), es.end());
    // position of an edge in spg_graph_get_edges order = number of live edges before it
    if (g->live_rank_stamp != g->n_mutations || g->live_rank.size() != g->edges.size()) {
        g->live_rank.resize(g->edges.size());
        int32_t r = 0;
        for (size_t e = 0; e < g->edges.size(); e++) { g->live_rank[e] = r; r += g->edges[e].alive ? 1 : 0; }
        g->live_rank_stamp = g->n_mutations;
    }
    int n = 0;
    for (int32_t e : es) { if (n < cap) edge_index[n] = g->live_rank[e]; n++; }
    return n;
}

// ================================================================================= debug hooks
// (tests) csrc/spg_internal.h
extern "C" int spg_debug_la(int op, int M, int N, int K, int flags, int mode, double *A, int ra, int lda, double *B, int rb, int ldb, double *C, int rc, int ldc, int *ok) {
    if (!A || !B || !C || !ok || M <= 0 || lda <= 0 || ldb <= 0 || ldc <= 0) return SPG_EINVAL;
    return spg::hip_la_test(op, M, N, K, flags, mode, A, ra, lda, B, rb, ldb, C, rc, ldc, ok);
}

extern "C" int spg_graph_last_blanket_count(const spg_graph *g) { return g ? (int)g->log.size() : 0; }
extern "C" int spg_graph_last_blankets(const spg_graph *g, int32_t *root_id, int32_t *round, int32_t *status, int32_t *info, double *kld, double *min_gap) {
    if (!g) return SPG_EINVAL;
    for (size_t i = 0; i < g->log.size(); i++) {
        if (root_id) root_id[i] = g->log[i].root_id;
        if (round) round[i] = g->log[i].round;
        if (status) status[i] = g->log[i].status;
        if (info) info[i] = g->log[i].info;
        if (kld) kld[i] = g->log[i].kld;
        if (min_gap) min_gap[i] = g->log[i].min_gap;
    }
    return (int)g->log.size();
}

// ================================================================================= batch entry
// Self-contained batch: builds a temporary arena [poses | edge records | out records | new slots |
// target infos], runs ONE round through the same backend entry the graph uses, unpacks the result.
extern "C" int spg_marginalize_batch(spg_ctx *ctx, const spg_options *o, const spg_batch *bt, spg_result *r) {
    if (!ctx || !o || !bt || !r) return SPG_EINVAL;
    const int d = o->pose_dim;
    if (d != 3 && d != 6) return SPG_EINVAL;
    const int ps = pose_stride(d);
    const int B = bt->B;
    r->new_edge_off[0] = 0;
    r->new_edge_vert_off[0] = 0;
    r->new_edge_data_off[0] = 0;
    if (B == 0) return 0;
    const int V = bt->vert_off[B], E = bt->edge_off[B];
    const int64_t ED = bt->edge_data_off[E];
    std::vector<double> host;
    int64_t o_pose = 0, o_edge = (int64_t)V * ps;
    int64_t cur = align_up(o_edge + ED, 32);
    std::vector<spg_blanket_desc> blk(B);
    std::vector<int64_t> vpo(V);
    std::vector<spg_edge_ref> er(E);
    for (int v = 0; v < V; v++) vpo[v] = o_pose + (int64_t)v * ps;
    for (int e = 0; e < E; e++) {
        er[e].off = o_edge + bt->edge_data_off[e];
        er[e].len = (int32_t)(bt->edge_data_off[e + 1] - bt->edge_data_off[e]);
        er[e].kind = bt->edge_kind[e];
        er[e].vbegin = bt->edge_vert_off[e];
        er[e].nv = bt->edge_vert_off[e + 1] - bt->edge_vert_off[e];
    }
    for (int b = 0; b < B; b++) {
        spg_blanket_desc &bd = blk[b];
        memset(&bd, 0, sizeof bd);
        bd.vert_begin = bt->vert_off[b];
        bd.n_vert = bt->vert_off[b + 1] - bt->vert_off[b];
        bd.n_remove = bt->n_remove[b];
        bd.edge_begin = bt->edge_off[b];
        bd.n_edge = bt->edge_off[b + 1] - bt->edge_off[b];
        int k = bd.n_vert - bd.n_remove;
        new_edge_budget(*o, d, std::max(k, 0), bd.n_new_max, bd.n_new_vert_max, bd.new_len);
        for (int e = bd.edge_begin; e < bd.edge_begin + bd.n_edge; e++)
            if (er[e].kind == SPG_EDGE_GLC) bd.pad_ = std::max(bd.pad_, er[e].len - d * er[e].nv + er[e].nv * 2 * d * d);
        bd.out_off = cur; cur += SPG_OUT_LEN(bd.n_new_max, bd.n_new_vert_max);
        bd.new_off = cur; cur += bd.new_len;
        if (r->target_info) { int64_t n = (int64_t)d * std::max(k, 0); bd.tinfo_off = cur; cur += n * n; }
        else bd.tinfo_off = -1;
    }
    int64_t in_len = align_up(o_edge + ED, 32);
    host.assign((size_t)cur, 0.0);
    memcpy(host.data(), bt->pose, (size_t)V * ps * 8);
    if (ED) memcpy(host.data() + o_edge, bt->edge_data, (size_t)ED * 8);
    void *dev = ctx->be.alloc(ctx->be.user, cur);
    if (!dev) return set_err(ctx, SPG_ENOMEM, "arena allocation failed");
    int rc = ctx->be.upload(ctx->be.user, dev, host.data(), in_len);
    spg_round_desc rd{};
    rd.opts = o;
    rd.n_blankets = B; rd.first = 0; rd.count = B;
    rd.blankets = blk.data();
    rd.vert_pose_off = vpo.data();
    rd.edges = er.data();
    rd.edge_vert = bt->edge_vert;
    rd.n_vert_total = V; rd.n_edge_total = E; rd.n_edge_vert_total = bt->edge_vert_off[E];
    if (!rc) rc = ctx->be.run_round(ctx->be.user, dev, &rd);
    if (!rc) rc = ctx->be.synchronize(ctx->be.user);
    if (!rc && cur > in_len) rc = ctx->be.download(ctx->be.user, host.data() + in_len, (char *)dev + in_len * 8, cur - in_len);
    ctx->be.release(ctx->be.user, dev);
    if (rc) {
        if (ctx->is_hip) copy_backend_error(ctx);
        return rc;
    }
    int32_t ne = 0, nev = 0;
    int64_t ned = 0;
    for (int b = 0; b < B; b++) {
        const spg_blanket_desc &bd = blk[b];
        const double *rec = host.data() + bd.out_off;
        r->status[b] = (int32_t)rec[0];
        if (r->info) r->info[b] = (int32_t)rec[1];
        r->kld[b] = rec[2];
        if (r->min_gap) r->min_gap[b] = rec[3];
        int n_new = (int)rec[4];
        int k = bd.n_vert - bd.n_remove;
        if (r->target_info && k > 0) {
            int64_t n = (int64_t)d * k;
            memcpy(r->target_info + r->target_info_off[b], host.data() + bd.tinfo_off, (size_t)(n * n) * 8);
        }
        int vpos = 0;
        for (int e = 0; e < n_new; e++) {
            int kind = (int)rec[SPG_OUT_HDR + 4 * e + 0];
            int64_t rel = (int64_t)rec[SPG_OUT_HDR + 4 * e + 1];
            int64_t len = (int64_t)rec[SPG_OUT_HDR + 4 * e + 2];
            int nv = (int)rec[SPG_OUT_HDR + 4 * e + 3];
            if (ne + 1 > r->new_edge_cap || nev + nv > r->new_edge_vert_cap || ned + len > r->new_edge_data_cap) return SPG_ECAPACITY;
            r->new_edge_kind[ne] = kind;
            for (int i = 0; i < nv; i++)
                r->new_edge_vert[nev++] = bt->vert_id[bd.vert_begin + (int)rec[SPG_OUT_HDR + 4 * bd.n_new_max + vpos + i]];
            vpos += nv;
            memcpy(r->new_edge_data + ned, host.data() + bd.new_off + rel, (size_t)len * 8);
            ned += len;
            ne++;
            r->new_edge_vert_off[ne] = nev;
            r->new_edge_data_off[ne] = ned;
        }
        r->new_edge_off[b + 1] = ne;
    }
    return 0;
}

// ================================================================================= substitute edge
// computeSubstituteEdge (src/compute_substitute_edge.cpp:13-96): online / cluster replay only. When a
// new edge points at a vertex that was already marginalised, walk breadth-first (ids <= maxid, never
// through vertex 0) to the nearest surviving vertex with the smallest id, compose the measurements
// along the way back and add the covariances. Host-side: 3x3 / 6x6 arithmetic once per such edge.
// Where the reference takes "the first edge of `reach` that touches the previous frontier" in g2o's
// pointer order, this build takes the lowest edge index.
namespace {
struct HPose { double t[3]; double q[4]; double th; };  // SE3: t,q ; SE2: t[0..1], th

void q_mul(const double *a, const double *b, double *o) {
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
void q_rot(const double *q, const double *v, double *o) {
    double x = q[0], y = q[1], z = q[2], w = q[3];
    double tx = 2 * (y * v[2] - z * v[1]), ty = 2 * (z * v[0] - x * v[2]), tz = 2 * (x * v[1] - y * v[0]);
    o[0] = v[0] + w * tx + (y * tz - z * ty);
    o[1] = v[1] + w * ty + (z * tx - x * tz);
    o[2] = v[2] + w * tz + (x * ty - y * tx);
}
double wrap_theta(double th) {
    const double PI = 3.14159265358979323846;
    if (th >= -PI && th < PI) return th;
    double m = std::fmod(th, 2 * PI);
    if (m >= PI) m -= 2 * PI;
    if (m < -PI) m += 2 * PI;
    return m;
}
}  // namespace
// (the two below also serve the spanning tree of spg_graph_initialize, spg_host_global.cpp: declared in spg_graph_impl.h)
void pose_compose(int d, const double *a, const double *b, double *o) {  // o = a * b (o may alias neither)
    if (d == 3) {
        double c = std::cos(a[2]), s = std::sin(a[2]);
        o[0] = a[0] + c * b[0] - s * b[1]; o[1] = a[1] + s * b[0] + c * b[1]; o[2] = wrap_theta(a[2] + b[2]);
    } else {
        double r[3];
        q_rot(a + 3, b, r);
        o[0] = a[0] + r[0]; o[1] = a[1] + r[1]; o[2] = a[2] + r[2];
        q_mul(a + 3, b + 3, o + 3);
        double n = std::sqrt(o[3] * o[3] + o[4] * o[4] + o[5] * o[5] + o[6] * o[6]);
        for (int i = 3; i < 7; i++) o[i] /= n;
    }
}
void pose_inverse(int d, const double *a, double *o) {
    if (d == 3) {
        double c = std::cos(a[2]), s = std::sin(a[2]);
        o[0] = -(c * a[0] + s * a[1]); o[1] = -(-s * a[0] + c * a[1]); o[2] = wrap_theta(-a[2]);
    } else {
        double qi[4] = {-a[3], -a[4], -a[5], a[6]}, r[3];
        q_rot(qi, a, r);
        o[0] = -r[0]; o[1] = -r[1]; o[2] = -r[2];
        o[3] = qi[0]; o[4] = qi[1]; o[5] = qi[2]; o[6] = qi[3];
    }
}
namespace {
bool dense_inverse(int n, std::vector<double> &A) {  // Gauss-Jordan, partial pivoting (Eigen .inverse())
    std::vector<double> X((size_t)n * n, 0.0);
    for (int i = 0; i < n; i++) X[(size_t)i * n + i] = 1.0;
    for (int k = 0; k < n; k++) {
        int p = k;
        for (int i = k + 1; i < n; i++) if (std::fabs(A[(size_t)i * n + k]) > std::fabs(A[(size_t)p * n + k])) p = i;
        if (A[(size_t)p * n + k] == 0.0) return false;
        if (p != k) for (int j = 0; j < n; j++) { std::swap(A[(size_t)k * n + j], A[(size_t)p * n + j]); std::swap(X[(size_t)k * n + j], X[(size_t)p * n + j]); }
        double ip = 1.0 / A[(size_t)k * n + k];
        for (int j = 0; j < n; j++) { A[(size_t)k * n + j] *= ip; X[(size_t)k * n + j] *= ip; }
        for (int i = 0; i < n; i++) {
            if (i == k) continue;
            double f = A[(size_t)i * n + k];
            if (f == 0.0) continue;
            for (int j = 0; j < n; j++) { A[(size_t)i * n + j] -= f * A[(size_t)k * n + j]; X[(size_t)i * n + j] -= f * X[(size_t)k * n + j]; }
        }
    }
    A.swap(X);
    return true;
}
}  // namespace

extern "C" int spg_graph_substitute_edge(spg_graph *g, const int32_t *marginalized, int n_marg, int maxid,
                                         int *from, int *to, double *meas, double *info_upper) {
    if (!g || !from || !to || !meas || !info_upper || (n_marg > 0 && !marginalized)) return SPG_EINVAL;
    if (int rc = sync_host(g)) return rc;
    const int d = g->d, ps = g->ps;
    const size_t NV = g->vid.size();
    auto slot_of = [&](int id) -> int32_t { auto it = g->vidx.find(id); return (it == g->vidx.end() || !g->valive[it->second]) ? -1 : it->second; };
    const int id_new = std::max(*from, *to), id_gone = std::min(*from, *to);   // the new vertex / its removed neighbour
    const int32_t s_new = slot_of(id_new), s_gone = slot_of(id_gone);
    if (s_new < 0 || s_gone < 0) return set_err(g->ctx, SPG_EINVAL, "substitute edge endpoint does not exist");
    // per-slot flags: bit 0 = removed so far, bit 1 = expanded by the search, bit 2 = queued for the next level
    std::vector<uint8_t> flag(NV, 0);
    for (int i = 0; i < n_marg; i++) { int32_t sl = slot_of(marginalized[i]); if (sl >= 0) flag[sl] |= 1; }
    // Breadth-first levels over vertex slots, every level in ascending id (the reference walks std::set<int>):
    // level[lvl_off[l] .. lvl_off[l+1]). A vertex that is removed (or an endpoint of the edge) is expanded; the
    // search stops at the first level that holds a surviving vertex and takes the smallest such id.
    std::vector<int32_t> level, lvl_off{0}, nextl;
    level.push_back(s_gone);
    lvl_off.push_back(1);
    flag[s_new] |= 2; flag[s_gone] |= 2;
    int32_t hit = -1;
    for (;;) {
        const int32_t lo = lvl_off[lvl_off.size() - 2], hi = lvl_off.back();
        nextl.clear();
        for (int32_t p = lo; p < hi; p++) {
            const int32_t v = level[p];
            const int id = g->vid[v];
            if (!(flag[v] & 1) && id != *from && id != *to) {
                if (hit < 0 || id < g->vid[hit]) hit = v;   // a survivor: candidate for the substitute endpoint
                continue;
            }
            flag[v] |= 2;
            for (int32_t eid : g->vr[v].adj) {
                const GEdge &e = g->edges[eid];
                if (e.nv != 2) continue;
                const int32_t u = (e.vtx[0] == v) ? e.vtx[1] : e.vtx[0];
                if ((flag[u] & 2) || g->vid[u] > maxid || g->vid[u] == 0 || (flag[u] & 4)) continue;
                flag[u] |= 4;
                nextl.push_back(u);
            }
        }
        if (hit >= 0) break;
        if (nextl.empty()) return set_err(g->ctx, SPG_EINVAL, "no surviving vertex reachable");
        std::sort(nextl.begin(), nextl.end(), [&](int32_t a, int32_t b) { return g->vid[a] < g->vid[b]; });
        for (int32_t u : nextl) flag[u] &= (uint8_t)~4;
        level.insert(level.end(), nextl.begin(), nextl.end());
        lvl_off.push_back((int32_t)level.size());
    }
    // Walk back from the survivor, level by level towards the new vertex: at each step the lowest-index pose-pose
    // edge of the current vertex that touches the previous level; measurements compose, covariances add.
    const int n_levels = (int)lvl_off.size() - 1;   // levels 0 .. n_levels-1; the survivor sits in the last one
    std::vector<double> cov((size_t)d * d, 0.0), acc(ps, 0.0), nxt(ps), zinv(ps), om((size_t)d * d);
    if (d == 6) acc[6] = 1.0;
    std::vector<uint8_t> in_prev(NV, 0);
    std::vector<int32_t> es;
    int32_t cur = hit;
    const bool new_is_from = (*from == id_new);
    for (int l = n_levels - 2; l >= -1; l--) {
        // previous level: l >= 0 -> the BFS level; l == -1 -> the new vertex alone
        if (l >= 0) for (int32_t p = lvl_off[l]; p < lvl_off[l + 1]; p++) in_prev[level[p]] = 1;
        else in_prev[s_new] = 1;
        es.assign(g->vr[cur].adj.begin(), g->vr[cur].adj.end());
        std::sort(es.begin(), es.end());
        bool stepped = false;
        for (int32_t eid : es) {
            const GEdge &e = g->edges[eid];
            if (e.nv != 2 || e.kind != SPG_EDGE_BINARY) continue;
            if (!(in_prev[e.vtx[0]] || in_prev[e.vtx[1]])) continue;
            const double *rec = g->host.data() + e.off;
            int q = 0;
            for (int i = 0; i < d; i++) for (int j = i; j < d; j++) { om[(size_t)i * d + j] = om[(size_t)j * d + i] = rec[ps + q]; q++; }
            if (!dense_inverse(d, om)) return set_err(g->ctx, SPG_EINVAL, "singular edge information on the substitute path");
            for (int i = 0; i < d * d; i++) cov[i] += om[i];
            const bool cur_is_head = (e.vtx[1] == cur);   // the edge points at the current vertex
            if (new_is_from) {
                if (cur_is_head) pose_compose(d, rec, acc.data(), nxt.data());
                else { pose_inverse(d, rec, zinv.data()); pose_compose(d, zinv.data(), acc.data(), nxt.data()); }
            } else {
                if (cur_is_head) { pose_inverse(d, rec, zinv.data()); pose_compose(d, acc.data(), zinv.data(), nxt.data()); }
                else pose_compose(d, acc.data(), rec, nxt.data());
            }
            acc.swap(nxt);
            cur = cur_is_head ? e.vtx[0] : e.vtx[1];
            stepped = true;
            break;
        }
        if (l >= 0) for (int32_t p = lvl_off[l]; p < lvl_off[l + 1]; p++) in_prev[level[p]] = 0;
        else in_prev[s_new] = 0;
        (void)stepped;   // as in the reference, a level without a matching edge is skipped
    }
    if (!dense_inverse(d, cov)) return set_err(g->ctx, SPG_EINVAL, "singular covariance sum");
    int q = 0;
    for (int i = 0; i < d; i++) for (int j = i; j < d; j++) info_upper[q++] = 0.5 * (cov[(size_t)i * d + j] + cov[(size_t)j * d + i]);
    for (int i = 0; i < ps; i++) meas[i] = acc[i];
    if (new_is_from) *to = g->vid[hit]; else *from = g->vid[hit];
    return 0;
}
