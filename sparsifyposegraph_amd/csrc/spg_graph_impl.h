// csrc/spg_graph_impl.h — the device-resident pose graph as the host translation units see it (spg_host.cpp: contexts,
// graph, I/O; spg_host_rounds.cpp: round scheduler and batch driver; spg_host_stream.cpp: streaming driver;
// spg_host_global.cpp: the whole-graph entry points) and what they share. Private: not part of include/spg.h.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#if defined(__linux__)
#include <pthread.h>
#include <sched.h>
#endif
#include <unistd.h>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include "../../include/spg.h"
#include "spg_internal.h"

namespace {
inline int pose_stride(int d) { return d == 3 ? 3 : 7; }
inline int info_len(int d) { return d * (d + 1) / 2; }
inline double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
inline void cpu_pause() {
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
}
// one turn of a wait for another thread: pause, and give the core away once the wait has become long
inline void spin_wait(uint32_t &spins) {
    if (++spins > 4096) std::this_thread::yield();
    else cpu_pause();
}
}  // namespace

// Host mirror of the arena: grows without value-initialising (the regions the device produces are
// never read before they are downloaded), unlike std::vector<double>::resize.
struct HostMirror {
    double *p = nullptr;
    size_t n = 0, cap = 0;
    ~HostMirror() { free(p); }
    HostMirror() {}
    HostMirror(const HostMirror &) = delete;
    HostMirror &operator=(const HostMirror &) = delete;
    double *data() { return p; }
    const double *data() const { return p; }
    size_t size() const { return n; }
    double &operator[](size_t i) { return p[i]; }
    const double &operator[](size_t i) const { return p[i]; }
    void resize(size_t m) {
        if (m > cap) {
            size_t nc = std::max(m, cap * 2);
            p = (double *)realloc(p, nc * sizeof(double));
            if (!p) abort();
            cap = nc;
        }
        n = m;
    }
};

// Small vector of trivially copyable T with N inline slots sharing their storage with the heap pointer of
// the spilled form: sizeof == 8 + N*sizeof(T), so per-vertex adjacency (N = 6 edge ids) and owner lists
// (N = 3 references) are one dense 32-byte record each instead of a vector header plus a heap chunk — the
// scheduler and the graph update are bound by the cache misses on exactly these lists.
template <class T, int N>
struct InlVec {
    int32_t n = 0, cap = N;
    union { T inl[N]; T *ptr; };
    InlVec() {}
    InlVec(const InlVec &o) : n(o.n), cap(o.cap) {
        if (cap > N) { ptr = (T *)malloc(sizeof(T) * (size_t)cap); memcpy(ptr, o.ptr, sizeof(T) * (size_t)n); }
        else memcpy(inl, o.inl, sizeof inl);
    }
    InlVec(InlVec &&o) noexcept : n(o.n), cap(o.cap) {
        if (cap > N) { ptr = o.ptr; o.cap = N; o.n = 0; }
        else memcpy(inl, o.inl, sizeof inl);
    }
    InlVec &operator=(InlVec o) noexcept {
        if (cap > N) free(ptr);
        n = o.n; cap = o.cap;
        if (cap > N) { ptr = o.ptr; o.cap = N; o.n = 0; }
        else memcpy(inl, o.inl, sizeof inl);
        return *this;
    }
    ~InlVec() { if (cap > N) free(ptr); }
    T *data() { return cap > N ? ptr : inl; }
    const T *data() const { return cap > N ? ptr : inl; }
    T *begin() { return data(); }
    T *end() { return data() + n; }
    const T *begin() const { return data(); }
    const T *end() const { return data() + n; }
    size_t size() const { return (size_t)n; }
    bool empty() const { return n == 0; }
    T &operator[](size_t i) { return data()[i]; }
    const T &operator[](size_t i) const { return data()[i]; }
    T &back() { return data()[n - 1]; }
    void pop_back() { n--; }
    void clear() { n = 0; }
    void push_back(const T &v) {
        if (n == cap) {
            int32_t nc = cap * 2;
            T *p = (T *)malloc(sizeof(T) * (size_t)nc);
            if (!p) abort();
            memcpy(p, data(), sizeof(T) * (size_t)n);
            if (cap > N) free(ptr);
            ptr = p; cap = nc;
        }
        data()[n++] = v;
    }
};

struct spg_ctx {
    spg_backend be{};
    bool is_hip = false;
    int rank = 0, nranks = 1;
    void *rccl = nullptr;         // communicator handle of csrc/spg_rccl.cpp (nullptr: single rank / no id given)
    int tag_counter = 0;          // ready tags are unique per context (its mailboxes are shared by all graphs)
    int linear_solver = 0;        // SPG_SOLVER_*: dense / block-sparse factorisation for optimize() and the global KLD
    double pcg_rel_tol = 0;       // spg_ctx_set_pcg; <= 0: the defaults (1e-10, min(n, 20000))
    int pcg_max_iter = 0;
    spg_pcg_stats pcg_stats{};    // of the last optimize call
    int greedy_method = 0;        // SPG_GREEDY_*: how select / prune get at Sigma (spg_ctx_set_greedy_method)
    int greedy_lookahead = 0;     // candidates per panel of the lazy rounds; 0: a full panel
    spg_greedy_stats greedy_stats{};   // of the last select / prune call that reached the device
    spg::StreamPort *sim_port = nullptr;   // tools/host_sim.cpp only: a simulated persistent worker behind an injected backend
    char err[768] = {0};
};

// 32 bytes (two per cache line, never straddling one); a pose-pose edge carries its two endpoints inline (vtx[0],
// vtx[1]) — the scheduler walks edges by the million and would otherwise take a second cache miss per edge for the
// endpoint list; an n-ary GLC edge keeps its vertices in spg_graph::everts at index vtx[0].
// `key` orders the edges of a blanket for the Hessian sum: the position the edge has in the REFERENCE's sequential
// execution (insertion order; edges created by a removal come after everything that existed when the call began, in
// removal-list order of their root, then in emission order) — the order g2o's edge set hands them out in the
// sequential loop, and independent of the order in which this library happens to commit commuting removals.
struct GEdge {
    int64_t off;
    int64_t key;
    int32_t len;
    int32_t vtx[2];
    int16_t nv;
    int8_t kind;
    uint8_t alive;
};

struct RoundBlanket {
    int32_t root;                 // vertex index
    int32_t n_remove;
    // flat pools (spg_graph::rb_verts / rb_edges) instead of per-blanket vectors: no allocation per blanket
    int32_t vbeg = 0, nv = 0;     // vertex indices, removed first (asc id) then kept (asc id)
    int32_t ebeg = 0, ne = 0;     // edge ids, ascending
    int32_t rank = 0;
    int32_t owner = -1;           // id in spg_graph::owners while the blanket is scheduled / in flight
    spg_blanket_desc desc{};
};

struct BlanketLog { int32_t root_id, round, status, info; double kld, min_gap; };

// One batch of mutually independent blankets: what used to be "the round". Two of them can be in
// flight on the two launch slots of the backend (the host prepares / commits one while the device
// computes the other).
struct Batch {
    std::vector<RoundBlanket> rb;
    std::vector<int32_t> rb_verts, rb_edges;
    std::vector<spg_blanket_desc> h_blk;
    std::vector<int64_t> h_vpo;
    std::vector<spg_edge_ref> h_er;
    std::vector<int32_t> h_ev;
    std::vector<int64_t> chunk_hdr;   // per rank: doubles of out records at the start of its chunk
    spg_round_info rinfo{};
    bool round_open = false;
    bool used_mailbox = false;
    int eff_ranks = 1, eff_rank = 0;   // ranks the batch is split over (1 = computed whole by every rank)
    int slot = 0;
    int seq = 0;                       // launch order
    int round_no = 0;
    int tag = 0;                       // ready tag of the launch (out record word [5])
    double t_launch = 0;               // SPG_TRACE=1 diagnostics
    // blankets committed from the mailbox before their KLD tail finished: (log index, mailbox offset)
    std::vector<std::pair<int32_t, int64_t>> kld_pending;
    // hand-over to the submission thread (pipelined driver): 0 while the batch's descriptors are being written and
    // handed to the device, 1 once that is done (submit_rc = result); a commit waits for 1
    alignas(64) std::atomic<int> submitted{1};
    int submit_rc = 0;
    char pad_[56];
};

struct OwnRefT { int32_t oid; uint32_t gen; };

struct spg_graph {
    spg_ctx *ctx = nullptr;
    int d = 0, ps = 0, rec = 0;
    std::vector<int32_t> vid;
    std::unordered_map<int32_t, int32_t> vidx;
    // direct id -> index table next to the hash map, kept while the ids are small non-negative integers (g2o files number
    // their vertices 0, 1, 2, ...): the 50 000 lookups of a removal list cost 2 ms of a 19 ms marginalisation through the map
    std::vector<int32_t> vdirect;
    bool vdirect_ok = true;
    int32_t index_of(int32_t id) const {
        if (vdirect_ok) return (id >= 0 && (size_t)id < vdirect.size()) ? vdirect[(size_t)id] : -1;
        auto it = vidx.find(id);
        return it == vidx.end() ? -1 : it->second;
    }
    std::vector<uint8_t> valive;
    std::vector<int64_t> vpose;
    // Per vertex, two cache lines. Line 0: adjacency — live edge ids, each with the far endpoint of a pose-pose edge
    // (-1 for an n-ary edge), so that walking a neighbourhood reads no edge records. Line 1: the streaming driver's
    // state of the vertex and what a hand-over needs of it (copies of vid[] / vpose[]).
    struct AdjEnt { int32_t eid, other; operator int32_t() const { return eid; } };
    struct SVtx {                                     // 24 bytes
        int32_t nown;                                 // registered blankets (in flight or reserved) that contain the vertex: own[0 .. nown)
        int32_t own[4];
        int32_t slot;                                 // SV_STABLE / SV_INFLIGHT: the slot that holds the vertex's blanket
    };
    struct alignas(64) VRec {
        InlVec<AdjEnt, 7> adj;
        SVtx s;
        int32_t id, pad_;
        int64_t pose;
        char spare_[24];
        VRec() { s.nown = 0; s.slot = -1; id = 0; pad_ = 0; pose = 0; }
    };
    std::vector<VRec> vr;
    std::vector<InlVec<struct OwnRefT, 3>> vown;      // batch scheduler: owners whose vertex set holds the vertex
    // list position and state of every vertex in one small array (4 bytes per vertex: it stays in L2 while the per-vertex
    // records stream through): -1 = not in the removal list of the running call, else (position << 2) | SV_*
    std::vector<int32_t> cst;
    std::vector<GEdge> edges;
    std::vector<int32_t> everts;
    int n_live_v = 0, n_live_e = 0;
    // arena
    void *dev = nullptr;
    int64_t cap = 0, used = 0;
    HostMirror host;               // mirror of [0, used)
    int64_t dev_synced = 0;        // device holds [0, dev_synced)
    int64_t stale_lo = 0, stale_hi = 0;  // host mirror range that only the device holds
    // marginalisation state
    bool active = false;
    spg_options opts{};
    int rank = 0, nranks = 1;
    std::vector<int32_t> pending;   // removal list (vertex indices) in the caller's order; [pend_head, end) is still to do
    size_t pend_head = 0;
    std::vector<uint8_t> in_set;   // vertex index is in the removal list
    static constexpr int NB = 8;                      // batches that can be in flight (= backend launch slots)
    Batch bt[NB];
    Batch *B = &bt[0];                                // batch the round functions currently work on
    // Owner registry of the scheduler: every scheduled-but-uncommitted blanket and every vertex deferred
    // in the current scheduling pass "owns" a vertex set; vowners[x] lists the owners whose set holds x.
    // Blanket owners persist from the pass that selected them until their batch commits; entries die
    // lazily: freeing an owner bumps its generation and stale references are dropped when next seen.
    struct Owner { int32_t batch, off, len; uint32_t gen; };   // batch >= 0: bt[batch].rb_verts[off, off+len); -1: Dpool
    using OwnRef = OwnRefT;
    std::vector<Owner> owners;
    std::vector<int32_t> owner_free, transient;       // free ids; deferred-vertex owners of the last pass
    std::vector<int32_t> Dpool;                       // sets of the deferred-vertex owners, flat
    int shard_threshold = -1;                         // < 0: cost model (shard_pays); >= 0: minimum blankets
    int round_no = 0, launch_seq = 0;
    bool pipelined = false;                           // two batches in flight (single rank, backend with slots)
    spg_marg_stats stats{};
    double tr_age = 0, tr_wait = 0, tr_first = 0; long tr_n = 0;   // SPG_TRACE=1: launch->commit-start, wait inside commit, launch->first ready word
    std::vector<BlanketLog> log;
    std::vector<double> hdr_buf;
    // Submission thread of the pipelined driver: the graph thread selects and commits, this one writes the descriptors
    // of a selected batch and hands it to the device (descriptor work + device hand-over are ~25 % of the host time per
    // batch and need nothing the graph thread mutates: poses, edge records' locations and the batch's own lists)
    // (every word the two threads exchange sits on its own cache line: the submission thread polls sub_tail, and a line
    //  shared with anything the graph thread writes per blanket would bounce between the cores all the time)
    std::thread sub_thread;
    static constexpr uint32_t SUBQ = 8;
    bool sub_active = false;
    struct alignas(64) SubShared {
        alignas(64) std::atomic<uint32_t> tail{0};    // written by the graph thread
        alignas(64) Batch *q[SUBQ] = {nullptr};       // written by the graph thread
        alignas(64) std::atomic<uint32_t> head{0};    // written by the submission thread
        alignas(64) double seconds = 0;               // submission thread only: time spent (descriptors + hand-over)
        alignas(64) std::atomic<bool> run{false};
        char pad_[64];
    } sub;
    std::vector<int32_t> live_rank;                   // edge id -> index among live edges (spg_graph_vertex_edges)
    long n_mutations = 0, live_rank_stamp = -1;       // bumped whenever an edge is added or dies
    // canonical edge keys (GEdge::key): next key for an edge added by the caller; base of the running marginalisation
    // (new edge e of the removal at list position p gets key_base + p * kKeyStride + e)
    int64_t next_key = 0, key_base = 0;
    static constexpr int64_t kKeyStride = 65536;
    std::vector<int32_t> lpos;                        // vertex index -> position in the removal list of the running call, -1 otherwise
    // scheduler scratch
    std::vector<int32_t> vstamp, estamp;
    int32_t stamp = 0;
    std::vector<int32_t> ocnt;
    std::vector<int32_t> lidx;
    std::vector<int32_t> s_newpending, s_B, s_centres, s_Dv, s_tmp, s_work, s_seen, s_hit, s_vix;
    std::vector<double> s_cost;
    std::vector<int> s_first;
    // ---- streaming driver (stream_marginalize below): per-vertex / per-slot / per-position state, kept between calls
    static constexpr int kSOwn = 4, kSMaxV = 16, kSMaxE = 44;
    struct SSlot {                                    // one blanket in flight
        int32_t pos, root, nv, ne, n_new_max, tag, logi, bell;
        int32_t launched;                             // 0: a reservation (the blanket of a waiting entry), 1: in flight
        int32_t npend, pend[3];                       // the blanket's other vertices that are list entries (-1: more than 3, look at all)
        int32_t mcell;                                // its mailbox cell: cells are handed out in launch order, so the host polls and reads sequential memory
        int64_t new_off, out_off;                     // out_off: emulated port only (out record in the arena), else -1
        int32_t verts[kSMaxV];                        // removed vertex first, kept ones in ascending id
        int32_t edges[kSMaxE];                        // ascending key
    };
    std::vector<SSlot> sslots;
    std::vector<int32_t> s_free, s_fifo, s_fin, s_woken, s_ready, wl_next, wl_stable, wl_done;
    int64_t unsorted_from = -1;                       // edges[unsorted_from ..) were appended in commit order by the streaming driver: see canonicalize_edge_order
    bool layout_diverged = false;                     // the graph has streamed on one of several ranks: its arena layout is rank-specific, never shard it again
    int stream_emulation = -1;                        // tests (spg_graph_set_stream_emulation): >= 0 = completion-order seed
    int stream_disabled = 0;                          // SPG_STREAM=0 or spg_graph_set_stream_emulation(g, -2)
    // robust kernel of spg_graph_optimize / _optimize_fixed (spg_graph_set_robust_kernel): SPG_ROBUST_*, width, and the
    // smallest vertex-id distance of the binary edges it applies to
    int robust_kind = 0, robust_gap = 1;
    double robust_delta = 1.0;
};

static inline const int32_t *edge_verts(const spg_graph *g, const GEdge &e) {
    return e.nv == 2 ? e.vtx : g->everts.data() + e.vtx[0];
}

inline int set_err(spg_ctx *c, int code, const char *fmt, const char *a = "") {
    if (c) snprintf(c->err, sizeof c->err, fmt, a);
    return code;
}

// ---- what crosses a unit boundary (library-internal: none of it is part of the exported ABI)
// spg_host.cpp
int sync_host(spg_graph *g);     // pull device-only ranges into the host mirror
int sync_device(spg_graph *g);   // push host-only tail to the device
void canonicalize_edge_order(spg_graph *g);
// The three above were already default-visibility symbols of the shared object; the ones below are shared for the first
// time and stay hidden, so that the library's dynamic symbol list does not grow.
#pragma GCC visibility push(hidden)
int arena_ensure(spg_graph *g, int64_t need);
int add_edge_idx(spg_graph *g, int kind, int nv, const int32_t *vix, int64_t off, int32_t len, int64_t key = -1);
// poses in arena layout (SE2: x y theta in [-pi, pi); SE3: t, unit quaternion x y z w)
void pose_compose(int d, const double *a, const double *b, double *o);   // o = a * b (o may alias neither)
void pose_inverse(int d, const double *a, double *o);
// spg_host_rounds.cpp
void quiesce_submission(spg_graph *g);   // wait until the submission thread has handed over every batch in its queue
// spg_host_stream.cpp
// Runs the removal list of the open marginalisation (spg_graph_marginalize_begin) through the streaming driver.
// Returns 0 = list exhausted, 1 = the rest of the list (g->pending from g->pend_head) is left to the batch driver
// (a blanket the persistent worker does not take, arena full, or no streaming on this backend), < 0 error.
int stream_marginalize(spg_graph *g, bool *started = nullptr);
#pragma GCC visibility pop

namespace {
inline void next_stamp(spg_graph *g) {
    if (g->vstamp.size() < g->vid.size()) g->vstamp.resize(g->vid.size(), 0);
    if (g->estamp.size() < g->edges.size()) g->estamp.resize(g->edges.size(), 0);
    g->stamp++;
}

// [lo, hi) of the arena was produced on the device: the host mirror does not hold it until sync_host
inline void mark_stale(spg_graph *g, int64_t lo, int64_t hi) {
    if (g->stale_hi <= g->stale_lo) { g->stale_lo = lo; g->stale_hi = hi; }
    else { g->stale_lo = std::min(g->stale_lo, lo); g->stale_hi = std::max(g->stale_hi, hi); }
}

// A live edge leaves the graph: the live flag, the counters (live_rank is rebuilt on the next use) and the adjacency
// entries of its vertices. What a committed blanket does to its edges and what spg_graph_remove_edges does.
inline void retire_edge(spg_graph *g, int32_t eid) {
    GEdge &e = g->edges[eid];
    e.alive = 0;
    g->n_mutations++;
    g->n_live_e--;
    for (int i = 0; i < e.nv; i++) {
        auto &av = g->vr[edge_verts(g, e)[i]].adj;
        for (size_t j = 0; j < av.size(); j++) if (av[j] == eid) { av[j] = av.back(); av.pop_back(); break; }
    }
}

// the HIP backend keeps the text of its last error: make it the context's
inline void copy_backend_error(spg_ctx *c) { snprintf(c->err, sizeof c->err, "%s", spg::hip_backend_error(&c->be)); }

// ---- out records ----------------------------------------------------------------------------------------------
// Word [5] of an out record against the tag of the launch that is to write it (include/spg.h at SPG_OUT_HDR): every
// poller of a mailbox asks this and nothing else.
enum MailState { MAIL_NOT_YET = 0, MAIL_READY = 1, MAIL_FINAL = 2 };
inline MailState mail_state(double word, double tag) {
    return word == SPG_READY_WORD(tag) ? MAIL_READY : word == SPG_FINAL_WORD(tag) ? MAIL_FINAL : MAIL_NOT_YET;
}

// (a full-format record comes from the device: nothing in it is used as an index before it has been checked)
// nv = vertices of the blanket the record belongs to
inline bool out_record_well_formed(const double *rec, const spg_blanket_desc &bd, int nv) {
    const int n_new = (int)rec[4];
    if (n_new < 0 || n_new > bd.n_new_max) return false;
    int vsum = 0;
    for (int e = 0; e < n_new; e++) {
        const double nvd = rec[SPG_OUT_HDR + 4 * e + 3], reld = rec[SPG_OUT_HDR + 4 * e + 1], lend = rec[SPG_OUT_HDR + 4 * e + 2];
        if (!(nvd >= 1 && nvd <= nv && reld >= 0 && lend >= 1 && reld + lend <= (double)bd.new_len)) return false;
        for (int i = 0; i < (int)nvd; i++) { const double li = rec[SPG_OUT_HDR + 4 * bd.n_new_max + vsum + i]; if (!(li >= 0 && li < nv)) return false; }
        vsum += (int)nvd;
        if (vsum > bd.n_new_vert_max) return false;
    }
    return true;
}
// The new edges of a full-format record: fn(e, kind, rel, len, nv, lv) — record at new_off + rel, `len` doubles;
// lv[0 .. nv) = the edge's vertices as indices into the blanket's vertex list.
template <class F>
inline void for_each_new_edge(const double *rec, int n_new, int n_new_max, F &&fn) {
    const double *lv = rec + SPG_OUT_HDR + 4 * n_new_max;
    for (int e = 0; e < n_new; e++) {
        const double *t = rec + SPG_OUT_HDR + 4 * e;
        const int nv = (int)t[3];
        fn(e, (int)t[0], (int64_t)t[1], (int32_t)t[2], nv, lv);
        lv += nv;
    }
}
// The new edges of a compact record (the persistent worker's, flags bit 20, spg_kernels.hip publish()): pose-pose
// edges only, endpoint pairs as 4-bit local indices, edge e in byte e of words [6] / [7]; their records lie back to
// back at new_off. fn(e, la, lb).
template <class F>
inline void for_each_compact_edge(const double *rec, int n_new, F &&fn) {
    uint64_t w[2];
    memcpy(w, rec + 6, 16);
    for (int e = 0; e < n_new; e++) {
        const unsigned pr = (unsigned)(w[e >> 3] >> (8 * (e & 7))) & 0xffu;
        fn(e, (int)(pr & 15u), (int)(pr >> 4));
    }
}

// ---- blanket descriptors ----------------------------------------------------------------------------------------
// most new edges / endpoints / record doubles a blanket with k kept vertices can emit
inline void new_edge_budget(const spg_options &o, int d, int k, int32_t &n_new_max, int32_t &n_new_vert_max, int64_t &new_len) {
    int ps = pose_stride(d);
    if (o.algorithm == SPG_ALG_NFR) {
        // pattern size (src/pseudo_chow_liu.cpp:33-87): a tree, or up to all pairs for Dense / Subgraph
        n_new_max = std::max(k - 1, 0);
        if (k > 2 && (o.topology == SPG_TOPO_DENSE || o.topology == SPG_TOPO_SUBGRAPH)) {
            const int msub = (int)((1 + o.chord_ratio) * (k - 1)), all = k * (k - 1) / 2;
            n_new_max = (o.topology == SPG_TOPO_DENSE || msub >= all) ? all : std::max(msub, k - 1);
        }
        n_new_vert_max = 2 * n_new_max;
        new_len = (int64_t)n_new_max * (ps + info_len(d));
        // correlated patterns: up to k - 1 measurements in all, possibly in one SPG_EDGE_MULTI record
        if (k > 2 && (o.topology == SPG_TOPO_CLIQUEY_SUBGRAPH || o.topology == SPG_TOPO_CLIQUEY_DENSE)) new_len += SPG_MULTI_LEN(d, k - 1);
    } else if (o.topology == SPG_TOPO_DENSE || k <= 1) {
        int64_t n = (int64_t)d * k;
        n_new_max = k > 0 ? 1 : 0;
        n_new_vert_max = k;
        new_len = n + n * n;
    } else {
        int64_t n2 = 2 * d;
        n_new_max = k;
        n_new_vert_max = 2 * k - 1;
        new_len = (d + (int64_t)d * d) + (int64_t)(k - 1) * (n2 + n2 * n2);
    }
}

// Appends the input side of one blanket's descriptor to a round's host arrays: its vertices' poses (verts: removed
// first, then kept), its edges' records and their vertices as indices into `verts` (through g->lidx, which must cover
// every vertex), and the assembly scratch its n-ary edges need. The output side of bd (new-edge budget, out_off /
// new_off) is the region layout's and stays with the caller. Reads only what no commit changes while the blanket is
// open: poses' offsets, the location / endpoints of existing edges.
inline void append_blanket_desc(spg_graph *g, const int32_t *verts, int nv, int n_remove, const int32_t *eids, int ne,
                                spg_blanket_desc &bd, std::vector<int64_t> &h_vpo, std::vector<spg_edge_ref> &h_er, std::vector<int32_t> &h_ev) {
    const int d = g->d;
    int32_t *const lidx = g->lidx.data();
    memset(&bd, 0, sizeof bd);
    bd.vert_begin = (int32_t)h_vpo.size();
    bd.n_vert = nv;
    bd.n_remove = n_remove;
    for (int i = 0; i < nv; i++) { h_vpo.push_back(g->vpose[verts[i]]); lidx[verts[i]] = (int32_t)i; }
    bd.edge_begin = (int32_t)h_er.size();
    bd.n_edge = ne;
    int32_t scratch = 0;
    for (int ei = 0; ei < ne; ei++) {
        const GEdge &e = g->edges[eids[ei]];
        if (e.kind == SPG_EDGE_GLC) scratch = std::max(scratch, e.len - d * e.nv + e.nv * 2 * d * d);
        spg_edge_ref er;
        er.off = e.off; er.len = e.len; er.kind = e.kind; er.vbegin = (int32_t)h_ev.size(); er.nv = e.nv;
        for (int i = 0; i < e.nv; i++) h_ev.push_back(lidx[edge_verts(g, e)[i]]);
        h_er.push_back(er);
    }
    bd.pad_ = scratch;  // doubles of assembly scratch the blanket's n-ary edges need (r*dq + q*2*d*d)
    bd.tinfo_off = -1;
}
}  // namespace
