// csrc/spg_host_stream.cpp — the streaming driver of libspg_hip.so.
//
// The batch driver (csrc/spg_host_rounds.cpp) hands the device ~50 blankets at a time and commits them as a unit; on graphs whose removals
// form long dependent chains (ring lattices: 250 rounds of 200) the host then idles while a batch is in flight and the
// device idles while the host commits and selects. Here ONE blanket is the unit: it is handed to the persistent worker
// kernel as one queue item the moment the rule below allows it, and committed the moment its ready word arrives,
// whatever else is in flight. Nothing is rescanned: a vertex that cannot go yet is parked on the ONE event that blocks
// it (an earlier vertex being launched, or being committed) and looked at again when that event happens.
//
// Rule. Positions are indices into the removal list; a vertex is WAITING, INFLIGHT (handed over, not committed) or DONE
// (committed: the host graph holds its effect). In the current host graph G, with X = N[v], WAITING v may be launched iff
//   (A) no vertex of X \ {v} is an earlier list entry that is not DONE (and none is INFLIGHT at all);
//   (B) for every x in X: every in-flight blanket that contains x contains no other vertex of X (and none contains v);
//       and no neighbour of any x in X \ {v} is an earlier WAITING list entry;
//   (C) no in-flight blanket of (B) that belongs to an earlier list entry contains a WAITING list entry earlier than v.
// Why this is the sequential result (src/vertex_remover.cpp:83-140 removes in list order): two removals commute when
// neither centre is in the other's blanket and the blankets share at most one vertex (header of spg_host_rounds.cpp). Take the
// earlier not-DONE entries in list order and assume the first one, u, whose blanket AT ITS TURN meets X in a vertex it
// does not meet now. The edge u - x it needs is created by a still earlier not-DONE removal whose blanket holds u and
// x; that one meets X, so it is one of the in-flight blankets seen in (B); u is in it, earlier than v and not INFLIGHT
// (an INFLIGHT vertex had no earlier not-DONE neighbour, (A)) — which (C) excludes. Hence the earlier removals that ever
// touch X are exactly the in-flight ones of (B), with frozen blankets sharing one vertex with X, and nothing earlier
// touches v, so X and its edges are what they will be at v's turn. (A vertex in flight was launched under the same
// rule, so later entries that run before v were checked against v from their side.)
// The earliest WAITING entry is only ever blocked by in-flight blankets, so the stream always makes progress.
// tests/test_stream_scheduler.py drives this code on the CPU with adversarial completion orders against the oracle.
#include "spg_graph_impl.h"

#if defined(__x86_64__)
#include <x86intrin.h>
static inline uint64_t ticks_now() { return __rdtsc(); }
#else
static inline uint64_t ticks_now() { return (uint64_t)(now_s() * 1e9); }
#endif

namespace {
enum : uint8_t { SV_WAITING = 0, SV_STABLE = 1, SV_INFLIGHT = 2, SV_DONE = 3 };
constexpr int kStreamSlots = 2048;       // blankets in flight at most (the worker has 256 workgroups; the rest queue)
constexpr int kStreamMailStride = 8;     // doubles per mailbox cell: the compact out record of the worker (flags bit 20, spg_kernels.hip publish()) is one cache line

// the blanket in slot s gives up its vertices (committed, or a reservation that was never launched)
__attribute__((always_inline)) inline void unregister_blanket(spg_graph *g, const int32_t s) {
    const spg_graph::SSlot &sl = g->sslots[s];
    spg_graph::VRec *const vr = g->vr.data();
    for (int i = 0; i < sl.nv; i++) {
        spg_graph::SVtx &sx = vr[sl.verts[i]].s;
        for (int j = 0; j < sx.nown; j++) if (sx.own[j] == s) { sx.own[j] = sx.own[--sx.nown]; break; }
    }
}

// Members in four groups: the rule and its state (examine, reserve, commit, harvest); the HIP transport (packets,
// doorbell, mailbox scan, poll helper thread); the emulated device of the CPU tests; run(), the loop over all of it.
struct Streamer {
    // ---------------------------------------------------------------------------------------------- rule state
    spg_graph *g;
    const bool emulate;
    const int D, ps, rec;
    const int32_t P;                     // list positions
    int32_t cursor = 0;                  // positions below it have been examined at least once
    int32_t prefetched_to = 0;
    int32_t n_done = 0, n_inflight = 0, pending_bell = 0, bell_no = 0;
    bool fallback = false;               // a blanket the worker does not take (or the arena is full): drain, then the batch driver
    int32_t cap_wait = -1;               // positions parked for a free slot
    uint64_t t_idle = 0;

    Streamer(spg_graph *g_, bool emu) : g(g_), emulate(emu), D(g_->d), ps(g_->ps), rec(g_->rec), P((int32_t)g_->pending.size()), arena_dev(g_->dev) {}

    struct SvView { spg_graph::VRec *vr; spg_graph::SVtx &operator[](int32_t i) const { return vr[i].s; } };

    long n_exam = 0, n_park[8] = {0};
    // SPG_STREAM_PROF=1: TSC ticks per phase (poll, commit, examine -> parked, examine -> launch decision, packet, doorbell, late results)
    const bool prof = [] { const char *e = getenv("SPG_STREAM_PROF"); return e && e[0] == '1'; }();
    uint64_t pt[8] = {0}, pn[8] = {0}, pt_last = 0;
    inline void P0() { if (prof) pt_last = ticks_now(); }
    inline void P1(int i) { if (prof) { const uint64_t n = ticks_now(); pt[i] += n - pt_last; pn[i]++; pt_last = n; } }
    void park(std::vector<int32_t> &heads, int32_t on, int32_t p) { g->wl_next[p] = heads[on]; heads[on] = p; }
    void wake(std::vector<int32_t> &heads, int32_t on) {
        for (int32_t p = heads[on]; p >= 0;) { const int32_t nx = g->wl_next[p]; g->s_woken.push_back(p); p = nx; }
        heads[on] = -1;
    }

    // index of y in X[0 .. nX) or -1. (Branch-free forms of this search, of the two small sorts and of the list removals were
    // measured on the bench workload: every one of them slower than the early-exit loops — 19.4 -> 20.6 -> 22.7 ms per step.)
    static inline int find(const int32_t *X, const int nX, const int32_t y) { for (int i = 0; i < nX; i++) if (X[i] == y) return i; return -1; }
    static inline void adj_remove(InlVec<spg_graph::AdjEnt, 7> &av, const int32_t eid) {
        for (size_t j = 0; j < av.size(); j++) if (av[j].eid == eid) { av[j] = av.back(); av.pop_back(); break; }
    }
    inline void set_pend(spg_graph::SSlot &sl, const int32_t *X, const int nX) {
        const int32_t *const cst = g->cst.data();
        sl.npend = 0;
        for (int i = 1; i < nX; i++) if (cst[X[i]] >= 0) { if (sl.npend == 3) { sl.npend = -1; break; } sl.pend[sl.npend++] = X[i]; }
    }
    // slot s holds the blanket X (X[0] = the vertex to remove) of list position p from now on, launched or reserved
    __attribute__((always_inline)) inline void register_blanket(const int32_t s, const int32_t p, const int32_t *X, const int nX) {
        const SvView sv{g->vr.data()};
        spg_graph::SSlot &sl = g->sslots[s];
        sl.pos = p; sl.root = X[0]; sl.nv = nX;
        memcpy(sl.verts, X, sizeof(int32_t) * (size_t)nX);
        set_pend(sl, X, nX);
        for (int i = 0; i < nX; i++) { spg_graph::SVtx &sx = sv[X[i]]; sx.own[sx.nown++] = s; }
    }

    // v passed (A): its blanket X is final as a vertex set. If it has to wait all the same, the set is registered like
    // the blanket of a launched vertex (a reservation), so that later entries are checked against it instead of waiting
    // for it; the slot becomes the blanket's own when it is launched. Without a free slot the vertex simply stays WAITING.
    void reserve(const int32_t p, const int32_t *X, const int nX) {
        const SvView sv{g->vr.data()};
        const int32_t v = X[0];
        if ((g->cst[v] & 3) != SV_WAITING || g->s_free.size() < 64) return;
        for (int i = 0; i < nX; i++) if (sv[X[i]].nown == spg_graph::kSOwn) return;
        const int32_t s = g->s_free.back(); g->s_free.pop_back();
        spg_graph::SSlot &sl = g->sslots[s];
        register_blanket(s, p, X, nX);
        sl.ne = 0; sl.launched = 0; sl.logi = -1;
        g->cst[v] = (p << 2) | SV_STABLE; sv[v].slot = s;
        if (g->wl_stable[p] >= 0) wake(g->wl_stable, p);
    }

    int examine(const int32_t p) {
        P0();
        const int r = examine_impl(p);
        P1(r ? 7 : 2);
        return r;
    }
    // 1 = launched, 0 = parked / nothing to do
    int examine_impl(const int32_t p) {
        const SvView sv{g->vr.data()};
        int32_t *const cst = g->cst.data();
        const int32_t v = g->pending[p];
        const int vstate = cst[v] & 3;
        if (vstate != SV_WAITING && vstate != SV_STABLE) return 0;
        n_exam++;
        spg_graph::VRec *const vr = g->vr.data();
        const GEdge *const edges = g->edges.data();
        const spg_graph::SSlot *const slots = g->sslots.data();
        int32_t X[spg_graph::kSMaxV];
        int nX = 1;
        int32_t mine = -1;                       // the slot of v's reservation
        if (vstate == SV_STABLE) {
            mine = sv[v].slot;
            nX = slots[mine].nv;
            memcpy(X, slots[mine].verts, sizeof(int32_t) * (size_t)nX);
        } else {
            X[0] = v;
            for (const spg_graph::AdjEnt &a : vr[v].adj) {
                const int32_t u = a.other;
                if (u < 0) { fallback = true; return 0; }   // an n-ary edge: not for the worker
                if (find(X, nX, u) < 0) {
                    if (nX == spg_graph::kSMaxV) { fallback = true; return 0; }
                    X[nX++] = u;
                }
            }
            const int k0 = nX - 1;
            if (k0 < 1 || D * k0 > spg::kWorkerMaxN) { fallback = true; return 0; }
            // (A)
            int32_t blocker = -1;   // of several blockers the LAST list entry: it is the one that finishes last, as a rule, and a wake-up by any other only parks v again
            for (int i = 1; i < nX; i++) {
                const int32_t c = cst[X[i]];
                // (a DONE entry that is still in the graph kept a status that forbids the graph update: it is inert)
                if (c >= 0 && (c & 3) != SV_DONE && ((c >> 2) < p || (c & 3) == SV_INFLIGHT)) blocker = std::max(blocker, c >> 2);
            }
            if (blocker >= 0) {
                n_park[0]++;
                park(g->wl_done, blocker, p);
                // first look at v (the list cursor runs well ahead of the results): pull what its launch will read — its
                // neighbours' records and its edges' records, cold in DRAM until now — towards the shared cache
                if (p >= prefetched_to) {
                    prefetched_to = p + 1;
                    __builtin_prefetch((const char *)&vr[v] + 64);
                    for (const spg_graph::AdjEnt &a : vr[v].adj) {
                        __builtin_prefetch(&edges[a.eid]);
                        __builtin_prefetch(&vr[a.other]);
                        __builtin_prefetch((const char *)&vr[a.other] + 64);
                    }
                }
                return 0;
            }
            // kept vertices in ascending id (buildSubgraph's order, src/vertex_remover.cpp:349-356)
            for (int i = 2; i < nX; i++) {
                const int32_t x = X[i], idx = vr[x].id;
                int j = i - 1;
                for (; j >= 1 && vr[X[j]].id > idx; j--) X[j + 1] = X[j];
                X[j + 1] = x;
            }
        }
        const int k = nX - 1;
        // (B), registered blankets (in flight, or reserved by an earlier entry that is itself waiting), and (C)
        for (int j = 0; j < sv[v].nown; j++) if (sv[v].own[j] != mine) { n_park[1]++; park(g->wl_done, slots[sv[v].own[j]].pos, p); return 0; }
        int32_t hs[spg_graph::kSMaxV * spg_graph::kSOwn];
        int nh = 0;
        for (int i = 1; i < nX; i++) {
            const spg_graph::SVtx &sx = sv[X[i]];
            for (int j = 0; j < sx.nown; j++) {
                const int32_t s = sx.own[j];
                if (s == mine) continue;
                if (!slots[s].launched && slots[s].pos > p) continue;   // a later entry's reservation: it is checked against v, not v against it
                for (int h = 0; h < nh; h++) if (hs[h] == s) { n_park[2]++; reserve(p, X, nX); park(g->wl_done, slots[s].pos, p); return 0; }
                hs[nh++] = s;
            }
        }
        {
            int32_t blocker = -1;
            for (int h = 0; h < nh; h++) {
                const spg_graph::SSlot &o = slots[hs[h]];
                if (o.pos > p) continue;
                const int32_t *mem = o.npend >= 0 ? o.pend : o.verts + 1;
                const int nmem = o.npend >= 0 ? o.npend : o.nv - 1;
                for (int i = 0; i < nmem; i++) {
                    const int32_t c = cst[mem[i]];
                    if (c >= 0 && (c & 3) == SV_WAITING && (c >> 2) < p) { blocker = std::max(blocker, o.pos); break; }
                }
            }
            if (blocker >= 0) { n_park[3]++; reserve(p, X, nX); park(g->wl_done, blocker, p); return 0; }
        }
        // (B), entries without a final blanket, fused with markovBlanketEdges (src/vertex_remover.cpp:225-251): one pass over
        // the adjacency of X \ {v}; no edge record is read (the far endpoints are in the adjacency entries) and no
        // per-vertex record of a vertex outside X (list positions and states come from the compact array)
        int32_t E[spg_graph::kSMaxE];
        int ne = 0;
        for (int i = 1; i < nX; i++) {
            for (const spg_graph::AdjEnt &a : vr[X[i]].adj) {
                const int32_t y = a.other;
                if (y < 0) { fallback = true; return 0; }
                const int j = find(X, nX, y);
                if (j >= 0) {
                    if (j == 0 || j >= i) {   // every blanket edge once: from its kept end, or from the lower-numbered of two kept ends
                        if (ne == spg_graph::kSMaxE) { fallback = true; return 0; }
                        E[ne++] = a.eid;
                    }
                } else {
                    const int32_t c = cst[y];
                    if (c >= 0 && (c & 3) == SV_WAITING && (c >> 2) < p) { n_park[4]++; reserve(p, X, nX); park(g->wl_stable, c >> 2, p); return 0; }
                }
            }
        }
        const int words = spg::kPktHdr + nX + 4 * ne;
        if (words > spg::kPktWords) { fallback = true; return 0; }
        if (mine < 0) {
            for (int i = 0; i < nX; i++) if (sv[X[i]].nown == spg_graph::kSOwn) { park(g->wl_done, slots[sv[X[i]].own[0]].pos, p); return 0; }
            if (g->s_free.empty()) { g->wl_next[p] = cap_wait; cap_wait = p; return 0; }
        }
        if (!emulate && cell_slot[launch_seq & (uint32_t)(port.slots - 1)] != -1) { g->wl_next[p] = cap_wait; cap_wait = p; return 0; }   // the next mailbox cell still holds an unharvested record
        // ---- launch
        const int n_new_max = k - 1, n_new_vert_max = 2 * (k - 1);
        const int64_t new_len = (int64_t)n_new_max * rec, out_len = emulate ? SPG_OUT_LEN(n_new_max, n_new_vert_max) : 0;
        if (g->used + new_len + out_len > g->cap) { fallback = true; return 0; }
        // ascending key = the reference's sequential edge order
        for (int i = 1; i < ne; i++) {
            const int32_t eid = E[i]; const int64_t key = edges[eid].key;
            int j = i - 1;
            for (; j >= 0 && edges[E[j]].key > key; j--) E[j + 1] = E[j];
            E[j + 1] = eid;
        }
        int32_t s = mine;
        if (s < 0) { s = g->s_free.back(); g->s_free.pop_back(); }
        spg_graph::SSlot &sl = g->sslots[s];
        if (mine < 0) register_blanket(s, p, X, nX);
        sl.ne = ne; sl.n_new_max = n_new_max; sl.logi = -1; sl.bell = bell_no + 1; sl.launched = 1;
        sl.tag = (++g->ctx->tag_counter & 0x3fffffff) + 1;
        sl.mcell = (int32_t)(launch_seq & (uint32_t)(port.slots - 1));
        if (!emulate) { cell_slot[sl.mcell] = s; launch_seq++; }
        sl.out_off = emulate ? g->used : -1;
        sl.new_off = g->used + out_len;
        g->used += new_len + out_len;
        memcpy(sl.edges, E, sizeof(int32_t) * (size_t)ne);
        cst[v] = (p << 2) | SV_INFLIGHT; sv[v].slot = s;
        P1(3);
        if (!emulate) build_packet(s, pending_bell);
        if (helper) hp.cell_tag[sl.mcell] = (uint32_t)sl.tag;
        P1(4);
        pending_bell++;
        n_inflight++;
        if (emulate) g->s_fifo.push_back(s);
        if (g->wl_stable[p] >= 0) wake(g->wl_stable, p);
        return 1;
    }

    // updateInputGraph (src/vertex_remover.cpp:500-546) for the blanket in slot s, whose out record is `recd`
    void commit(const int32_t s, const double *recd, const bool final_seen) {
        spg_graph::SSlot &sl = g->sslots[s];
        const int32_t p = sl.pos, v = sl.root;
        const int status = (int)recd[0], inf = (int)recd[1], n_new = (int)recd[4];
        sl.logi = (int32_t)g->log.size();
        g->log.push_back({g->vid[v], sl.bell, status, inf, recd[2], recd[3]});
        g->stats.max_blanket = std::max(g->stats.max_blanket, sl.nv);
        const bool fine = (status == SPG_OK || status == SPG_ST_KLD_NOT_PD);
        if (!fine) g->stats.n_bad_status++;
        else {
            for (int i = 0; i < sl.ne; i++) {
                const int32_t eid = sl.edges[i];
                GEdge &e = g->edges[eid];
                e.alive = 0;
                adj_remove(g->vr[e.vtx[0]].adj, eid);
                if (e.vtx[1] != e.vtx[0]) adj_remove(g->vr[e.vtx[1]].adj, eid);
            }
            g->n_mutations += sl.ne + 1;
            g->n_live_e -= sl.ne;
            g->valive[v] = 0;
            g->vr[v].adj.clear();
            g->n_live_v--;
            g->stats.n_removed++;
            const int64_t key0 = g->key_base + (int64_t)p * spg_graph::kKeyStride;
            if (!emulate) {
                for_each_compact_edge(recd, n_new, [&](int e, int la, int lb) {
                    const int32_t va = sl.verts[la], vb = sl.verts[lb];
                    // (add_edge_idx for a pose-pose edge between two different vertices, without its general-case checks)
                    GEdge ge;
                    ge.off = sl.new_off + (int64_t)e * rec; ge.key = key0 + e; ge.len = rec; ge.vtx[0] = va; ge.vtx[1] = vb; ge.nv = 2; ge.kind = SPG_EDGE_BINARY; ge.alive = 1;
                    const int32_t eid = (int32_t)g->edges.size();
                    g->edges.push_back(ge);
                    g->vr[va].adj.push_back({eid, vb});
                    if (vb != va) g->vr[vb].adj.push_back({eid, va});
                });
            } else {
                for_each_new_edge(recd, n_new, sl.n_new_max, [&](int e, int kind, int64_t rel, int32_t len, int, const double *lv) {
                    int32_t vix[2] = {sl.verts[(int)lv[0]], sl.verts[(int)lv[1]]};
                    add_edge_idx(g, kind, 2, vix, sl.new_off + rel, len, key0 + e);
                });
            }
            g->stats.n_new_edges += n_new;
            if (!emulate) { g->n_mutations += n_new; g->n_live_e += n_new; }
        }
        unregister_blanket(g, s);
        g->cst[v] = (p << 2) | SV_DONE;
        n_done++;
        n_inflight--;
        if (final_seen) harvest(s, recd);
        else g->s_fin.push_back(s);
        if (g->wl_done[p] >= 0) wake(g->wl_done, p);
    }
    // the KLD tail of a committed blanket has landed (final word): late results, then the slot is free again
    void harvest(const int32_t s, const double *recd) {
        spg_graph::SSlot &sl = g->sslots[s];
        BlanketLog &lg = g->log[sl.logi];
        lg.kld = recd[2]; lg.min_gap = recd[3]; lg.status = (int32_t)recd[0];
        if (std::isfinite(recd[2])) g->stats.kld_sum += recd[2];
        if (!emulate) cell_slot[sl.mcell] = -1;
        g->s_free.push_back(s);
        for (int32_t q = cap_wait; q >= 0;) { const int32_t nx = g->wl_next[q]; g->s_woken.push_back(q); q = nx; }
        cap_wait = -1;
    }

    // ------------------------------------------------------------------------------------------- HIP transport
    // The poll helper re-reads port.h_mail / mail_stride / slots on every scan. The port and arena_dev fill one cache line
    // of their own, which the graph thread writes once per doorbell (port.tail); what it writes per launch starts on the next.
    alignas(64) spg::StreamPort port;
    void *arena_dev;
    static_assert(sizeof(spg::StreamPort) + sizeof(void *) == 64, "port + arena_dev = the cache line the poll helper reads");
    uint32_t launch_seq = 0, poll_seq = 0;  // blankets launched so far; the oldest launch whose result has not been taken
    std::vector<int32_t> cell_slot;         // mailbox cell -> slot of the blanket whose record it holds / will hold, -1 = free, -2 = taken (committed, not harvested)
    double alg_bytes = 0;

    // The queue item of the blanket in slot s (layout: spg_kernels.hip, blanket_worker), written through the BAR, and its
    // item word; `ahead` = items written since the last doorbell. Reads the slot, the poses' offsets and the blanket
    // edges' records' locations (all immutable once the slot is handed over).
    void build_packet(const int32_t s, const int ahead) {
        const spg_graph::SSlot &sl = g->sslots[s];
        const spg_graph::VRec *const vr = g->vr.data();
        const GEdge *const edges = g->edges.data();
        const int nX = sl.nv, ne = sl.ne, n_new_max = sl.n_new_max;
        const int words = spg::kPktHdr + nX + 4 * ne;
        unsigned long long pkt[spg::kPktWords];
        auto pack = [](int lo, int hi) { return (unsigned long long)(uint32_t)lo | ((unsigned long long)(uint32_t)hi << 32); };
        const spg_options &o = g->opts;
        pkt[0] = (unsigned long long)(uintptr_t)arena_dev;
        pkt[1] = port.d_mail;
        pkt[2] = 0;
        pkt[3] = (unsigned long long)((int64_t)sl.mcell * port.mail_stride); pkt[4] = (unsigned long long)sl.new_off; pkt[5] = (unsigned long long)(int64_t)-1;
        pkt[6] = pack(nX, 1); pkt[7] = pack(ne, n_new_max); pkt[8] = pack(2 * n_new_max, 0);
        pkt[9] = pack(o.topology, o.flags | (1 << 20)); pkt[10] = pack(o.lin_point, sl.tag);   // bit 20: compact out record
        memcpy(&pkt[11], &o.chord_ratio, 8);
        pkt[12] = pack(words, 2 * ne);
        int w = spg::kPktHdr;
        for (int i = 0; i < nX; i++) pkt[w++] = (unsigned long long)vr[sl.verts[i]].pose;
        int32_t *evp = (int32_t *)(pkt + spg::kPktHdr + nX + 3 * ne);
        double by = 8.0 * ps * nX + 12.0 + 8.0 * (double)n_new_max * rec;
        for (int i = 0; i < ne; i++) {
            const GEdge &e = edges[sl.edges[i]];
            spg_edge_ref er;
            er.off = e.off; er.len = e.len; er.kind = e.kind; er.vbegin = 2 * i; er.nv = 2;
            memcpy(&pkt[w], &er, 24);
            w += 3;
            evp[2 * i] = find(sl.verts, nX, e.vtx[0]); evp[2 * i + 1] = find(sl.verts, nX, e.vtx[1]);
            by += 8.0 + 8.0 * e.len;
        }
        alg_bytes += by;
        unsigned long long *dst = port.pkt + (size_t)s * spg::kPktWords;
        memcpy(dst, pkt, (size_t)words * 8);                                                  // through the BAR (write-combined)
        port.q->item[(port.tail + (unsigned long long)ahead) % spg::kQCap] = (unsigned long long)(uintptr_t)dst;
    }

    void ring() {
        if (!pending_bell) return;
        P0();
        if (!emulate) {
            std::atomic_thread_fence(std::memory_order_release);
#if defined(__x86_64__)
            __builtin_ia32_sfence();   // packets and item words have left the write-combining buffers before the doorbell
#endif
            port.tail += (unsigned long long)pending_bell;
            for (int c = 0; c < port.bells; c++) port.q->tail[c * spg::kBellStride] = port.tail;
#if defined(__x86_64__)
            __builtin_ia32_sfence();
#endif
        }
        pending_bell = 0;
        bell_no++;
        g->stats.n_batches++;
        if (helper) hp.launches.store(launch_seq, std::memory_order_release);
        P1(5);
    }

    inline const double *cell(int32_t s) const { return port.h_mail + (size_t)g->sslots[s].mcell * (size_t)port.mail_stride; }

    // The scan of the mailbox cells of launches [from, to). Cells are handed out in launch order and tickets are served
    // in that order, so results land nearly in sequence in sequential memory: the scan stops after `giveup` unfinished
    // cells in a row. pending(cell, tag): a handle >= 0 if a result is still to come in that cell, and the tag it will
    // carry; take(q, handle, final): the result of launch q has arrived. Both callers' closures are inlined.
    template <class Pending, class Take>
    inline void scan_mailbox(const uint32_t from, const uint32_t to, const int giveup, Pending &&pending, Take &&take) const {
        const uint32_t mask = (uint32_t)(port.slots - 1);
        int misses = 0;
        for (uint32_t q0 = from; q0 != to && misses < giveup;) {
            // the ready words of the next 16 cells are loaded before any is looked at: the lines the device has just written
            // miss the caches, and behind a branch per cell those misses would be taken one after the other
            const uint32_t nq = std::min<uint32_t>(16, to - q0);
            double w[16];
            for (uint32_t i = 0; i < nq; i++) w[i] = ((const volatile double *)(port.h_mail + (size_t)((q0 + i) & mask) * (size_t)port.mail_stride))[5];
            for (uint32_t i = 0; i < nq; i++) {
                const uint32_t q = q0 + i;
                double tagd;
                const int32_t h = pending(q & mask, tagd);
                if (h < 0) continue;
                const MailState st = mail_state(w[i], tagd);
                if (st != MAIL_NOT_YET) { take(q, h, st == MAIL_FINAL); misses = 0; }
                else misses++;
            }
            q0 += nq;
        }
    }

    // Blankets whose ready (or final) word has arrived, on the graph thread: the scan starts at the oldest launch not
    // taken yet (every 16th call looks at everything in flight).
    void poll_hip(int giveup) {
        std::vector<int32_t> &ready = g->s_ready;
        const uint32_t mask = (uint32_t)(port.slots - 1);
        while (poll_seq != launch_seq && cell_slot[poll_seq & mask] < 0) poll_seq++;
        scan_mailbox(poll_seq, launch_seq, giveup,
                     [&](uint32_t cell, double &tagd) -> int32_t {
                         const int32_t s = cell_slot[cell];
                         if (s >= 0) tagd = (double)g->sslots[s].tag;
                         return s;
                     },
                     [&](uint32_t q, int32_t s, bool) {
                         __builtin_prefetch(&g->sslots[s]); __builtin_prefetch((const char *)&g->sslots[s] + 64); __builtin_prefetch((const char *)&g->sslots[s] + 128);
                         ready.push_back(s);
                         cell_slot[q & mask] = -2;
                     });
        // the ready words the next call will look at first: on their way while this call's results are committed (a cell the
        // device has not written yet comes in stale and is invalidated by the write; one it has written is a hit next time)
        {
            uint32_t q = poll_seq;
            for (int n = 0; q != launch_seq && n < 12; q++) {
                if (cell_slot[q & mask] < 0) continue;
                __builtin_prefetch((const void *)(port.h_mail + (size_t)(q & mask) * (size_t)port.mail_stride));
                n++;
            }
        }
    }

    // ---- poll helper (on by default for lists of 4096 entries or more; SPG_STREAM_THREADS=1 switches it off): a second host thread does nothing but watch the
    // mailbox and copy each record that has arrived — one cache line — into a ring of ordinary memory, so that the graph
    // thread reads results from the neighbouring core's cache instead of taking a miss on device-written memory per poll.
    // It touches no graph data: all it needs is the number of launches so far and the tag each cell will show.
    struct Helper {
        static constexpr uint32_t RQ = 4096;
        alignas(64) std::atomic<uint32_t> launches{0};   // graph thread: cells [0, launches) have been handed out (their tags are in cell_tag)
        alignas(64) std::atomic<uint32_t> r_tail{0};     // helper: results published
        alignas(64) std::atomic<int> stop{0};
        alignas(64) uint32_t r_head = 0;                  // graph thread
        std::vector<double> rq;                           // RQ entries of 8 doubles: the compact record, word [5] = 2 * launch number + final flag
        std::vector<uint32_t> cell_tag;
        char pad_[64];
    } hp;
    bool helper = false;
    std::thread helper_thread;
    std::vector<const double *> ready_rec;               // helper mode: ring entry of each slot in g->s_ready

    void helper_main() {
        const uint32_t mask = (uint32_t)(port.slots - 1);
        std::vector<uint8_t> pend((size_t)port.slots, 0);
        uint32_t head = 0, seen = 0, r_tail = 0;
        unsigned n = 0;
        while (!hp.stop.load(std::memory_order_acquire)) {
            const uint32_t lp = hp.launches.load(std::memory_order_acquire);
            while (seen != lp) { pend[seen & mask] = 1; seen++; }
            while (head != seen && !pend[head & mask]) head++;
            const int giveup = (++n & 15) ? 10 : 1 << 20;
            bool got = false;
            scan_mailbox(head, seen, giveup,
                         [&](uint32_t cell, double &tagd) -> int32_t {
                             if (!pend[cell]) return -1;
                             tagd = (double)hp.cell_tag[cell];
                             return (int32_t)cell;
                         },
                         [&](uint32_t q, int32_t cell, bool final) {
                             double *e = hp.rq.data() + (size_t)(r_tail & (Helper::RQ - 1)) * 8;
                             memcpy(e, port.h_mail + (size_t)cell * (size_t)port.mail_stride, 64);
                             e[5] = (double)(2.0 * (double)q + (final ? 1.0 : 0.0));
                             r_tail++;
                             pend[cell] = 0;
                             got = true;
                         });
            if (got) hp.r_tail.store(r_tail, std::memory_order_release);
        }
    }
    void take_helper_results() {
        const uint32_t rt = hp.r_tail.load(std::memory_order_acquire);
        const uint32_t mask = (uint32_t)(port.slots - 1);
        ready_rec.clear();
        while (hp.r_head != rt) {
            const double *e = hp.rq.data() + (size_t)(hp.r_head & (Helper::RQ - 1)) * 8;
            __builtin_prefetch(e + 8); __builtin_prefetch(e + 16);
            const uint32_t q = (uint32_t)((uint64_t)e[5] >> 1);
            const int32_t s = cell_slot[q & mask];
            g->s_ready.push_back(s);
            ready_rec.push_back(e);
            cell_slot[q & mask] = -2;
            __builtin_prefetch(&g->sslots[s]); __builtin_prefetch((const char *)&g->sslots[s] + 64); __builtin_prefetch((const char *)&g->sslots[s] + 128);
            hp.r_head++;
        }
    }
    // The helper is only used when it can sit on a core that shares an L3 with this thread's (cores of a group of 8 do on
    // the hosts this runs on) and both can be pinned for the duration of the call: across L3s the ring costs more than the
    // polls it saves. Returns false (nothing started) otherwise.
    bool helper_start() {
#if defined(__linux__)
        static const bool pin = [] { const char *e = getenv("SPG_PIN_THREADS"); return !(e && e[0] == '0'); }();
        if (!pin || sched_getaffinity(0, sizeof old_mask, &old_mask) != 0) return false;
        const int cpu = sched_getcpu();
        int cand = -1;
        for (int d = 1; cpu >= 0 && d < 8 && cand < 0; d++) {
            const int c = (cpu & ~7) | ((cpu + d) & 7);
            if (c < CPU_SETSIZE && CPU_ISSET(c, &old_mask)) cand = c;
        }
        if (cand < 0) return false;
        cpu_set_t one; CPU_ZERO(&one); CPU_SET(cpu, &one);
        if (sched_setaffinity(0, sizeof one, &one) != 0) return false;
        repin = true;
        hp.rq.resize((size_t)Helper::RQ * 8);
        hp.cell_tag.assign((size_t)port.slots, 0);
        helper = true;
        helper_thread = std::thread([this] { helper_main(); });
        CPU_ZERO(&one); CPU_SET(cand, &one);
        (void)pthread_setaffinity_np(helper_thread.native_handle(), sizeof one, &one);
        return true;
#else
        return false;
#endif
    }
    void helper_stop() {
        if (!helper) return;
        hp.stop.store(1, std::memory_order_release);
        helper_thread.join();
        helper = false;
#if defined(__linux__)
        if (repin) (void)sched_setaffinity(0, sizeof old_mask, &old_mask);
#endif
    }
#if defined(__linux__)
    cpu_set_t old_mask;
    bool repin = false;
#endif

    // ----------------------------------------------------------------------------------------- emulated device
    size_t fifo_head = 0;
    uint64_t rng;
    // Emulated device (injected backend; tests): "complete" a subset of the in-flight blankets, chosen and ordered by the
    // seed, by running them as one round of the backend; their out records land in the arena.
    int poll_emulated() {
        std::vector<int32_t> &fifo = g->s_fifo, &ready = g->s_ready;
        std::vector<int32_t> live;
        for (size_t i = fifo_head; i < fifo.size(); i++) if (fifo[i] >= 0) live.push_back((int32_t)i);
        if (live.empty()) { fifo.clear(); fifo_head = 0; return 0; }
        auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
        size_t take = live.size();
        if (g->stream_emulation > 0) {
            take = 1 + (size_t)(next() % live.size());
            for (size_t i = 0; i + 1 < live.size(); i++) std::swap(live[i], live[i + (size_t)(next() % (live.size() - i))]);
        }
        live.resize(take);
        std::vector<spg_blanket_desc> blk(take);
        std::vector<int64_t> vpo;
        std::vector<spg_edge_ref> er;
        std::vector<int32_t> ev;
        for (size_t t = 0; t < take; t++) {
            const spg_graph::SSlot &sl = g->sslots[fifo[live[t]]];
            spg_blanket_desc &bd = blk[t];
            append_blanket_desc(g, sl.verts, sl.nv, 1, sl.edges, sl.ne, bd, vpo, er, ev);
            bd.n_new_max = sl.n_new_max; bd.n_new_vert_max = 2 * sl.n_new_max;
            bd.new_off = sl.new_off; bd.new_len = (int64_t)sl.n_new_max * rec; bd.out_off = sl.out_off;
        }
        spg_round_desc rd{};
        rd.opts = &g->opts; rd.n_blankets = (int32_t)take; rd.first = 0; rd.count = (int32_t)take;
        rd.blankets = blk.data(); rd.vert_pose_off = vpo.data(); rd.edges = er.data(); rd.edge_vert = ev.data();
        rd.n_vert_total = (int64_t)vpo.size(); rd.n_edge_total = (int64_t)er.size(); rd.n_edge_vert_total = (int64_t)ev.size();
        rd.mail_base = 0; rd.mail_len = 0; rd.slot = 0; rd.tag = ++g->ctx->tag_counter;
        if (int r = g->ctx->be.run_round(g->ctx->be.user, g->dev, &rd)) return r;
        if (int r = g->ctx->be.synchronize(g->ctx->be.user)) return r;
        for (size_t t = 0; t < take; t++) {
            const int32_t s = fifo[live[t]];
            const spg_graph::SSlot &sl = g->sslots[s];
            const int64_t olen = SPG_OUT_LEN(sl.n_new_max, 2 * sl.n_new_max);
            if (int r = g->ctx->be.download(g->ctx->be.user, g->host.data() + sl.out_off, (char *)g->dev + sl.out_off * 8, olen)) return r;
            ready.push_back(s);
            fifo[live[t]] = -1;
        }
        while (fifo_head < fifo.size() && fifo[fifo_head] < 0) fifo_head++;
        return 0;
    }

    // ----------------------------------------------------------------------------------------------------- run
    std::vector<int32_t> &woken = g->s_woken, &ready = g->s_ready, &fin = g->s_fin;
    size_t fin_head = 0;                 // fin[fin_head ..): committed blankets whose final word has not been taken
    unsigned n_polls = 0;
    uint64_t last_progress = 0, idle_since = 0;

    // results that have arrived, into `ready` (helper mode: their ring entries into ready_rec)
    int take_results() {
        ready.clear();
        P0();
        if (emulate) { if (int r = poll_emulated()) return r; }
        else if (n_inflight) {
            if (helper) take_helper_results(); else poll_hip((++n_polls & 15) ? 10 : 1 << 20);
        }
        P1(0);
        return 0;
    }
    // every result that has arrived is committed before anything is examined: a woken entry often waits for two or
    // three of them (its column's predecessor and that one's neighbours), and looking at it between their commits
    // only parks it again
    void commit_ready() {
        for (size_t ri = 0; ri < ready.size(); ri++) {
            const int32_t s = ready[ri];
            const double *recd = emulate ? g->host.data() + g->sslots[s].out_off : (helper ? ready_rec[ri] : cell(s));
            const bool fin_now = emulate || (helper ? (((uint64_t)recd[5]) & 1) != 0 : mail_state(recd[5], g->sslots[s].tag) == MAIL_FINAL);
            P0();
            commit(s, recd, fin_now);
            P1(1);
        }
    }
    // woken entries are examined in list order: an earlier one that launches (or gets its final blanket) is often
    // what a later one of the same wake-up waits for — the wait lists hand them out newest first
    void examine_woken() {
        if (!fallback) {
            if (woken.size() > 1) std::sort(woken.begin(), woken.end());
            for (size_t wi = 0; wi < woken.size(); wi++) {
                examine(woken[wi]);
                if (pending_bell >= 8) ring();
            }
        }
        woken.clear();
    }
    // late results (final words) of committed blankets, in bulk: each is a line the device has rewritten since the
    // commit read it (a miss), nothing waits for them, and taken 64 at a time the misses overlap
    void late_results() {
        if (emulate || !(fin.size() - fin_head >= 192 || g->s_free.size() < 256 || (cap_wait >= 0 && fin_head < fin.size()))) return;
        P0();
        const size_t n = std::min<size_t>(64, fin.size() - fin_head);
        for (size_t i = 0; i < n; i++) __builtin_prefetch((const void *)cell(fin[fin_head + i]));
        for (size_t i = 0; i < n; i++) {
            const int32_t s = fin[fin_head];
            const volatile double *c = cell(s);
            if (mail_state(c[5], g->sslots[s].tag) != MAIL_FINAL) break;
            harvest(s, (const double *)c);
            fin_head++;
        }
        if (fin_head > 8192) { fin.erase(fin.begin(), fin.begin() + (long)fin_head); fin_head = 0; }
        P1(6);
        if (!woken.empty()) {
            if (!fallback) for (size_t wi = 0; wi < woken.size(); wi++) examine(woken[wi]);
            woken.clear();
        }
    }
    // list entries nobody has looked at yet: a few per turn, more when the device leaves the host idle
    void advance_cursor(const bool got) {
        if (fallback || cursor >= P) return;
        int budget = got ? 4 : 32;
        while (cursor < P && budget-- > 0 && !fallback) {
            examine(cursor++);
            if (!woken.empty()) { for (size_t wi = 0; wi < woken.size() && !fallback; wi++) examine(woken[wi]); woken.clear(); }
        }
    }
    // nothing arrived and nothing to examine: the host waits for the device. 0 = go on waiting, 1 = leave through the
    // batch driver, < 0 error
    int idle_check() {
        const uint64_t t1 = ticks_now();
        if (!idle_since) idle_since = t1;
        if (n_inflight == 0 && fin_head == fin.size()) {
            // nothing in flight, list not exhausted, nothing woken: every remaining entry is parked on an entry that never
            // ran — cannot happen (the earliest WAITING entry only waits for blankets in flight); leave through the batch driver
            fallback = true;
            return 1;
        }
        if (((t1 - last_progress) >> 35) != 0) {   // ~ 10 s without a result
            set_err(g->ctx, SPG_EHIP, "streaming driver: no blanket completed within 10 s");
            return SPG_EHIP;
        }
        return 0;
    }
    // every committed blanket's final word (its slot, packet and mailbox cell are reused by the next call)
    int drain() {
        if (!emulate) {
            const double t0 = now_s();
            for (; fin_head < fin.size(); fin_head++) {
                const int32_t s = fin[fin_head];
                const volatile double *c = cell(s);
                uint32_t spins = 0;
                while (mail_state(c[5], g->sslots[s].tag) != MAIL_FINAL) {
                    if ((++spins & 0xfff) == 0 && now_s() - t0 > 10.0) { set_err(g->ctx, SPG_EHIP, "streaming driver: a blanket's KLD tail did not complete within 10 s"); return SPG_EHIP; }
                    cpu_pause();
                }
                harvest(s, (const double *)c);
            }
            woken.clear();
        }
        fin.clear();
        return 0;
    }
    void account(const uint64_t t_begin, const double s_begin) {
        if (idle_since) { t_idle += ticks_now() - idle_since; idle_since = 0; }
        const uint64_t t_end = ticks_now();
        const double secs = now_s() - s_begin;
        const double idle = (t_end > t_begin) ? secs * (double)t_idle / (double)(t_end - t_begin) : 0.0;
        g->stats.device_seconds += idle;
        g->stats.host_seconds += secs - idle;
        g->stats.schedule_seconds += secs - idle;   // (selection, commit and hand-over are one loop here; SPG_STREAM_PROF splits them)
        if (prof) {
            const char *nm[8] = {"poll", "commit", "examine: parked", "examine: launch decision", "packet", "doorbell", "late results", "launch tail"};
            const double tps = (double)(t_end - t_begin) / secs;
            for (int i = 0; i < 8; i++) fprintf(stderr, "stream prof %-26s %8llu x %8.1f ns = %8.3f ms\n", nm[i], (unsigned long long)pn[i], pn[i] ? 1e9 * (double)pt[i] / tps / (double)pn[i] : 0.0, 1e3 * (double)pt[i] / tps);
        }
    }

    int run() {
        const uint64_t t_begin = ticks_now();
        const double s_begin = now_s();
        last_progress = t_begin;
        for (;;) {
            if (int r = take_results()) return r;
            const bool got = !ready.empty();
            if (got && idle_since) { t_idle += ticks_now() - idle_since; idle_since = 0; }
            commit_ready();
            examine_woken();
            late_results();
            advance_cursor(got);
            ring();
            if (n_done == P) break;
            if (fallback && n_inflight == 0) break;
            if (got || cursor < P) { last_progress = ticks_now(); continue; }
            if (int r = idle_check()) { if (r < 0) return r; break; }
        }
        if (int r = drain()) return r;
        account(t_begin, s_begin);
        return 0;
    }
};
}  // namespace

// (what it returns: csrc/spg_graph_impl.h)
int stream_marginalize(spg_graph *g, bool *started) {
    const spg_options &o = g->opts;
    if (started) *started = false;
    static const bool env_off = [] { const char *e = getenv("SPG_STREAM"); return e && e[0] == '0'; }();
    spg::StreamPort *const sim = g->ctx->is_hip ? nullptr : g->ctx->sim_port;
    const bool emulate = !g->ctx->is_hip && !sim;
    if (env_off || g->stream_disabled) return 1;
    if (emulate && g->stream_emulation < 0) return 1;
    if (g->nranks != 1 || o.algorithm != SPG_ALG_NFR || o.topology != SPG_TOPO_TREE || o.lin_point != SPG_LIN_GLOBAL || (o.flags & ~SPG_FLAG_NFR_FACTOR_DESCENT) != 0) return 1;
    const int32_t P = (int32_t)g->pending.size();
    if (P < (emulate ? 1 : 64)) return 1;   // a handful of removals (online decimation): one plain launch is cheaper than starting the worker
    Streamer S(g, emulate);
    if (sim) {
        if (sim->slots < kStreamSlots || sim->mail_stride < kStreamMailStride) return 1;
        S.port = *sim;
    } else if (!emulate) {
        int prc = spg::hip_stream_open(&g->ctx->be, g->d, kStreamSlots, kStreamMailStride, &S.port);
        if (prc < 0) { copy_backend_error(g->ctx); return prc; }
        if (prc > 0) return 1;
    }
    // state
    const size_t V = g->vid.size();
    if (g->cst.size() < V) g->cst.resize(V, -1);
    for (int32_t p = 0; p < P; p++) { g->cst[g->pending[p]] = (p << 2) | SV_WAITING; g->vr[g->pending[p]].s.nown = 0; }
    g->wl_next.assign((size_t)P, -1); g->wl_stable.assign((size_t)P, -1); g->wl_done.assign((size_t)P, -1);
    if (g->sslots.size() < (size_t)kStreamSlots) g->sslots.resize(kStreamSlots);
    g->s_free.clear();
    for (int s = kStreamSlots - 1; s >= 0; s--) g->s_free.push_back(s);
    g->s_fifo.clear(); g->s_fin.clear(); g->s_woken.clear(); g->s_ready.clear();
    next_stamp(g);
    if (g->lidx.size() < V) g->lidx.resize(V, -1);
    if ((int64_t)g->host.size() < g->cap) g->host.resize((size_t)g->cap);
    S.rng = 0x9E3779B97F4A7C15ULL ^ ((uint64_t)(g->stream_emulation > 0 ? g->stream_emulation : 1) * 0xD1B54A32D192ED03ULL);
    const int64_t used0 = g->used;
    if (started) *started = true;
    if (g->unsorted_from < 0) g->unsorted_from = (int64_t)g->edges.size();
    if (!emulate) S.cell_slot.assign((size_t)S.port.slots, -1);
    // second host thread that only polls the mailbox (SPG_STREAM_THREADS=1: none); the simulated port of tools/host_sim.cpp
    // gets one only on request (=2): its "device" is a thread as well
    static const int want_helper = [] { const char *e = getenv("SPG_STREAM_THREADS"); return e ? atoi(e) : 0; }();
    if (!emulate && (want_helper == 2 || (want_helper == 0 && !sim)) && P >= 4096) (void)S.helper_start();
    const double t_setup = now_s();
    const int rc = S.run();
    S.helper_stop();
    const double t_ran = now_s();
    if (sim) sim->tail = S.port.tail;
    else if (!emulate) spg::hip_stream_close(&g->ctx->be, &S.port, S.alg_bytes, (long long)S.n_done);
    // what the stream produced in the arena is device-only until someone asks for it
    if (g->used > used0) {
        g->dev_synced = g->used;
        if (!emulate && !sim) mark_stale(g, used0, g->used);
        else {
            // injected backend: the mirror is filled from the backend's arena right away (tests read edges next)
            if (int r = g->ctx->be.download(g->ctx->be.user, g->host.data() + used0, (char *)g->dev + used0 * 8, g->used - used0)) return r;
        }
    }
    g->stats.n_rounds = S.bell_no;
    g->round_no = S.bell_no;
    // list entries the stream did not finish, in list order, for the batch driver
    size_t left = 0;
    for (int32_t p = 0; p < P; p++) {
        const int32_t v = g->pending[p];
        spg_graph::SVtx &sq = g->vr[v].s;
        const int vst = g->cst[v] & 3;
        if (vst == SV_STABLE) unregister_blanket(g, sq.slot);   // a reservation that was never launched (the stream handed over to the batch driver)
        const bool done = vst == SV_DONE;
        g->cst[v] = -1; sq.nown = 0;
        if (!done) g->pending[left++] = v;
    }
    g->pending.resize(left);
    g->pend_head = 0;
    if (getenv("SPG_TRACE")) {
        fprintf(stderr, "spg trace: streaming driver: run %.3f ms, tear-down %.3f ms\n", 1e3 * (t_ran - t_setup), 1e3 * (now_s() - t_ran));
        fprintf(stderr, "spg trace: streaming driver: %d list entries, %d committed in %d doorbells, %zu left to the batch driver (examined up to entry %d)\n",
                P, S.n_done, S.bell_no, left, S.cursor);
        fprintf(stderr, "spg trace: streaming driver: %ld examinations; parked on: earlier neighbour %ld, own blanket %ld, two shared vertices %ld, waiting member of a touching blanket %ld, waiting 2-hop neighbour %ld\n",
                S.n_exam, S.n_park[0], S.n_park[1], S.n_park[2], S.n_park[3], S.n_park[4]);
    }
    if (rc) return rc;
    return left ? 1 : 0;
}

// tools/host_sim.cpp (declared in csrc/spg_internal.h, not part of the public ABI): the streaming driver of a context
// with an injected backend talks to this port — host memory, with a thread of the tool playing the persistent worker.
extern "C" int spg_debug_set_stream_port(spg_ctx *c, void *port) {
    if (!c || c->is_hip) return SPG_EINVAL;
    c->sim_port = (spg::StreamPort *)port;
    return 0;
}

extern "C" int spg_graph_set_stream_emulation(spg_graph *g, int seed) {
    if (!g) return SPG_EINVAL;
    g->stream_disabled = seed <= -2;
    g->stream_emulation = seed < 0 ? -1 : seed;
    return 0;
}
