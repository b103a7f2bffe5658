// csrc/spg_graph_impl.h — the device-resident pose graph as the host translation units see it (spg_host.cpp: graph,
// scheduler, drivers; spg_host_global.cpp: the whole-graph entry points). Private: not part of include/spg.h.
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
    std::vector<int64_t> s_chunk_len;
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
};

static inline const int32_t *edge_verts(const spg_graph *g, const GEdge &e) {
    return e.nv == 2 ? e.vtx : g->everts.data() + e.vtx[0];
}

inline int set_err(spg_ctx *c, int code, const char *fmt, const char *a = "") {
    if (c) snprintf(c->err, sizeof c->err, fmt, a);
    return code;
}

// spg_host.cpp
int sync_host(spg_graph *g);     // pull device-only ranges into the host mirror
int sync_device(spg_graph *g);   // push host-only tail to the device
void canonicalize_edge_order(spg_graph *g);
