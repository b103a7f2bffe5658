// csrc/spg_host_rounds.cpp — the conflict-free round scheduler and the batch driver of libspg_hip.so: the round calls
// of include/spg.h (begin / prepare / compute / commit / end), the pipelined loop over them and its optional submission
// thread. The streaming driver it hands suitable removal lists to is csrc/spg_host_stream.cpp.
//
// Sequential semantics. VertexRemover::remove mutates the graph after every vertex
// (src/vertex_remover.cpp:134). Two removals commute exactly when neither centre lies in the other's
// blanket and the blankets share at most one vertex (then no existing or future edge can belong to
// both). Each round scans the pending list in the reference's order and selects a vertex only if it
// commutes with every earlier vertex that is selected in this round or still deferred — a deferred
// vertex is represented by a superset D(u) of every vertex its blanket can reach before its turn.
#include "spg_graph_impl.h"

// ================================================================================= scheduler
// N[v] including v (markovBlanketVertices, src/vertex_remover.cpp:197-215); unsorted, deduplicated
static void closed_neighbourhood(spg_graph *g, int32_t v, std::vector<int32_t> &out) {
    next_stamp(g);
    out.clear();
    out.push_back(v);
    g->vstamp[v] = g->stamp;
    for (int32_t eid : g->vr[v].adj) {
        const GEdge &e = g->edges[eid];
        for (int i = 0; i < e.nv; i++) {
            int32_t u = edge_verts(g, e)[i];
            if (g->vstamp[u] != g->stamp) { g->vstamp[u] = g->stamp; out.push_back(u); }
        }
    }
}

// extendedMarkovBlanketVertices (src/vertex_remover.cpp:142-195), literal: one ascending pass over
// the growing id-ordered set; pick bin = every vertex of the removal list that is still alive.
static void extended_blanket(spg_graph *g, int32_t root, std::vector<int32_t> &verts, std::vector<int32_t> &picked) {
    auto byid = [g](int32_t a, int32_t b) { return g->vid[a] < g->vid[b]; };
    std::set<int32_t, decltype(byid)> ret(byid), pk(byid);
    std::vector<int32_t> tmp;
    closed_neighbourhood(g, root, tmp);
    ret.insert(tmp.begin(), tmp.end());
    pk.insert(root);
    for (auto it = ret.begin(); it != ret.end(); ++it) {
        int32_t v = *it;
        if (g->in_set[v] && !pk.count(v)) {
            pk.insert(v);
            closed_neighbourhood(g, v, tmp);
            ret.insert(tmp.begin(), tmp.end());
        }
    }
    verts.assign(ret.begin(), ret.end());
    picked.assign(pk.begin(), pk.end());
}

static bool dense_mode(const spg_options &o) { return o.topology == SPG_TOPO_DENSE || o.topology == SPG_TOPO_CLIQUEY_DENSE; }

// markovBlanketEdges (src/vertex_remover.cpp:225-251) for a selected blanket. `verts` must be stamped.
static void collect_edges(spg_graph *g, const int32_t *verts, int nverts, const std::vector<int32_t> &centres,
                          bool intra, std::vector<int32_t> &out) {
    next_stamp(g);
    int32_t st = g->stamp;
    for (int i = 0; i < nverts; i++) g->vstamp[verts[i]] = st;
    out.clear();
    for (int vi_ = 0; vi_ < nverts; vi_++) {
        int32_t v = verts[vi_];
        for (int32_t eid : g->vr[v].adj) {
            if (g->estamp[eid] == st) continue;
            g->estamp[eid] = st;
            const GEdge &e = g->edges[eid];
            bool ok = true, hub = false;
            for (int i = 0; i < e.nv; i++) {
                int32_t u = edge_verts(g, e)[i];
                if (g->vstamp[u] != st) { ok = false; break; }
                if (!intra) for (int32_t c : centres) hub |= (c == u);
            }
            if (ok && (intra || hub)) out.push_back(eid);
        }
    }
    // (ascending key = the reference's sequential edge order, whatever order commuting removals were committed in)
    std::sort(out.begin(), out.end(), [g](int32_t a, int32_t b) { return g->edges[a].key < g->edges[b].key; });
}

static int32_t owner_acquire(spg_graph *g, int32_t batch, int32_t off, int32_t len) {
    int32_t oid;
    if (!g->owner_free.empty()) { oid = g->owner_free.back(); g->owner_free.pop_back(); }
    else { oid = (int32_t)g->owners.size(); g->owners.push_back({0, 0, 0, 0}); g->ocnt.push_back(0); }
    spg_graph::Owner &o = g->owners[oid];
    o.batch = batch; o.off = off; o.len = len;
    return oid;
}
static void owner_release(spg_graph *g, int32_t oid) {
    g->owners[oid].gen++;   // every reference to it in vowners[] is stale from now on
    g->owner_free.push_back(oid);
}
static const int32_t *owner_set(const spg_graph *g, const spg_graph::Owner &o) {
    return (o.batch >= 0 ? g->bt[o.batch].rb_verts.data() : g->Dpool.data()) + o.off;
}
static void release_batch_owners(spg_graph *g, Batch &bt) {
    for (RoundBlanket &r : bt.rb) if (r.owner >= 0) { owner_release(g, r.owner); r.owner = -1; }
}

// Select this round's mutually commuting blankets, in list order. Fills bt.rb; rewrites g->pending.
#ifdef SPG_SCHED_PROF
#include <x86intrin.h>
static unsigned long long prof_t[16], prof_n[16];
#define PT0 unsigned long long pt_ = __rdtsc()
#define PT(i) do { unsigned long long n_ = __rdtsc(); prof_t[i] += n_ - pt_; prof_n[i]++; pt_ = n_; } while (0)
#else
#define PT0 do {} while (0)
#define PT(i) do {} while (0)
#endif
static void schedule_round(spg_graph *g) {
    Batch &bt = *g->B;
    const spg_options &o = g->opts;
    const bool dense = dense_mode(o);
    const size_t DCAP = 512;
    bt.rb.clear();
    bt.rb_verts.clear();
    bt.rb_edges.clear();
    // the deferred-vertex owners of the previous pass are void; blanket owners of batches still in
    // flight stay registered (their removals are not in the host graph yet, so nothing that fails to
    // commute with them may be selected now)
    for (int32_t oid : g->transient) owner_release(g, oid);
    g->transient.clear();
    g->Dpool.clear();
    const int32_t my_batch = (int32_t)(&bt - g->bt);
    // scratch that keeps its capacity between passes (a pass runs a thousand times per marginalisation)
    std::vector<int32_t> &newpending = g->s_newpending, &B = g->s_B, &centres = g->s_centres, &Dv = g->s_Dv, &tmp = g->s_tmp,
                         &work = g->s_work, &seen_owner = g->s_seen, &hit = g->s_hit;
    newpending.clear();
    bool stop = false;
    size_t n_deferred = 0, consec = 0;
    auto reg = [&](int32_t batch, int32_t off, int32_t len) -> int32_t {
        int32_t oid = owner_acquire(g, batch, off, len);
        const uint32_t gen = g->owners[oid].gen;
        const int32_t *set = owner_set(g, g->owners[oid]);
        for (int32_t i = 0; i < len; i++) g->vown[set[i]].push_back({oid, gen});
        return oid;
    };
    // live owners of x, dropping stale references on the way
    auto for_owners = [&](int32_t x, auto &&fn) {
        auto &vo = g->vown[x];
        for (size_t i = 0; i < vo.size();) {
            const spg_graph::OwnRef r = vo[i];
            if (g->owners[r.oid].gen != r.gen) { vo[i] = vo.back(); vo.pop_back(); continue; }
            fn(r.oid);
            i++;
        }
    };
    bool inflight = false;
    for (int bi = 0; bi < spg_graph::NB; bi++) inflight |= (&g->bt[bi] != &bt && g->bt[bi].round_open);
    // The scan touches only a prefix of the pending list: entries that have to wait are written back
    // right in front of the untouched tail, so a call costs O(scanned), not O(pending).
    size_t pos = g->pend_head;
    for (; pos < g->pending.size() && !stop; pos++) {
        int32_t v = g->pending[pos];
        if (!g->valive[v]) continue;  // absorbed by an earlier cluster (`deleted`, src/vertex_remover.cpp:91)
        PT0;
        if (dense) extended_blanket(g, v, B, centres);
        else { closed_neighbourhood(g, v, B); centres.assign(1, v); }
        PT(0);
        bool inD = false, conflict = false;
        hit.clear();
        for (int32_t x : B) {
            bool is_c = false;
            for (int32_t c : centres) is_c |= (c == x);
            for_owners(x, [&](int32_t oid) {
                if (is_c) inD = true;
                if (g->ocnt[oid]++ == 0) hit.push_back(oid);
                if (g->ocnt[oid] >= 2) conflict = true;
            });
        }
        for (int32_t oid : hit) g->ocnt[oid] = 0;
        PT(1);
        if (!inD && !conflict) {
            RoundBlanket rbk;
            rbk.root = v;
            rbk.n_remove = (int32_t)centres.size();
            auto byid = [g](int32_t a, int32_t b) { return g->vid[a] < g->vid[b]; };
            std::sort(centres.begin(), centres.end(), byid);
            tmp.clear();
            for (int32_t x : B) {
                bool is_c = false;
                for (int32_t c : centres) is_c |= (c == x);
                if (!is_c) tmp.push_back(x);
            }
            std::sort(tmp.begin(), tmp.end(), byid);
            rbk.vbeg = (int32_t)bt.rb_verts.size();
            bt.rb_verts.insert(bt.rb_verts.end(), centres.begin(), centres.end());
            bt.rb_verts.insert(bt.rb_verts.end(), tmp.begin(), tmp.end());
            rbk.nv = (int32_t)(centres.size() + tmp.size());
            PT(5);
            collect_edges(g, bt.rb_verts.data() + rbk.vbeg, rbk.nv, centres, o.include_intra_clique != 0, work);
            rbk.ebeg = (int32_t)bt.rb_edges.size();
            rbk.ne = (int32_t)work.size();
            bt.rb_edges.insert(bt.rb_edges.end(), work.begin(), work.end());
            PT(6);
            rbk.owner = reg(my_batch, rbk.vbeg, rbk.nv);
            bt.rb.push_back(std::move(rbk));
            consec = 0;
            PT(2);
        } else {
            newpending.push_back(v);
            n_deferred++;
            // D(v): everything v's blanket can reach before its turn
            next_stamp(g);
            int32_t st = g->stamp;
            Dv.clear();
            auto addv = [&](int32_t x) { if (g->vstamp[x] != st) { g->vstamp[x] = st; Dv.push_back(x); } };
            for (int32_t x : B) addv(x);
            work.assign(centres.begin(), centres.end());
            size_t wi = 0;
            seen_owner.clear();
            while (wi < work.size() && Dv.size() <= DCAP) {
                int32_t c = work[wi++];
                for_owners(c, [&](int32_t oid) {
                    bool seen = false;
                    for (int32_t so : seen_owner) seen |= (so == oid);
                    if (seen) return;
                    seen_owner.push_back(oid);
                    const spg_graph::Owner ow = g->owners[oid];
                    for (int32_t yi = 0; yi < ow.len; yi++) {
                        int32_t y = owner_set(g, ow)[yi];   // (re-resolved: work/addv never touch the pools)
                        bool fresh = g->vstamp[y] != st;
                        addv(y);
                        // Dense: a newly reachable removable vertex is itself absorbed and brings its neighbourhood
                        if (dense && fresh && g->in_set[y] && g->valive[y]) work.push_back(y);
                    }
                });
                if (dense && c != v) {
                    // neighbourhood of an absorbed vertex (stamps are in use: gather without closed_neighbourhood)
                    for (int32_t eid : g->vr[c].adj) {
                        const GEdge &e = g->edges[eid];
                        for (int i = 0; i < e.nv; i++) {
                            int32_t y = edge_verts(g, e)[i];
                            bool fresh = g->vstamp[y] != st;
                            addv(y);
                            if (fresh && g->in_set[y] && g->valive[y]) work.push_back(y);
                        }
                    }
                }
            }
            if (Dv.size() > DCAP) { stop = true; continue; }  // (v is already in newpending; the loop ends here)
            {
                int32_t off = (int32_t)g->Dpool.size();
                g->Dpool.insert(g->Dpool.end(), Dv.begin(), Dv.end());
                g->transient.push_back(reg(-1, off, (int32_t)Dv.size()));
            }
            // stop scanning once a long run of list entries had to wait: whatever follows is
            // (almost always) waiting on them too, and not scanning only defers more
            // (with another batch in flight the blocked stretch is usually exactly the part of the list
            //  that waits for it: give up sooner, the next call comes right after that batch commits)
            static const int pat_inflight = [] { const char *e = getenv("SPG_PATIENCE"); return e ? atoi(e) : 16; }();
            size_t patience = inflight ? pat_inflight + bt.rb.size() / 16 : 48 + bt.rb.size() / 8;
            if (++consec > patience || n_deferred > 256 + 2 * bt.rb.size()) stop = true;
            PT(3);
        }
    }
    {
        size_t nd = newpending.size();
        size_t nh = pos - nd;
        for (size_t i = 0; i < nd; i++) g->pending[nh + i] = newpending[i];
        g->pend_head = nh;
    }
}

// ================================================================================= rounds
extern "C" int spg_graph_marginalize_begin(spg_graph *g, const int32_t *which, int n, const spg_options *opts, int rank, int nranks) {
    if (!g || !opts || (n > 0 && !which) || nranks < 1 || rank < 0 || rank >= nranks) return SPG_EINVAL;
    if (g->active) return set_err(g->ctx, SPG_ESTATE, "marginalize already in progress");
    if (opts->pose_dim != g->d) return set_err(g->ctx, SPG_EINVAL, "pose_dim mismatch");
    g->opts = *opts;
    g->rank = rank; g->nranks = nranks;
    g->pending.clear();
    g->pend_head = 0;
    g->in_set.assign(g->vid.size(), 0);
    g->lpos.assign(g->vid.size(), -1);
    for (int i = 0; i < n; i++) {
        const int32_t vi = g->index_of(which[i]);
        if (vi < 0 || !g->valive[vi])
            return set_err(g->ctx, SPG_EINVAL, "vertex needs to exist in order to be marginalized");
        if (g->in_set[vi]) continue;
        g->in_set[vi] = 1;
        g->lpos[vi] = (int32_t)g->pending.size();
        g->pending.push_back(vi);
    }
    // keys of the edges this call creates: after everything that exists, ordered by list position of their root
    g->key_base = g->next_key;
    g->next_key = g->key_base + ((int64_t)g->pending.size() + 1) * spg_graph::kKeyStride;
    // room for the regions of the rounds to come (grown later if this estimate is short). An arena that was reserved for
    // the job (spg_graph_reserve: 2.5x or more of what is in use) is left alone: growing means a new allocation, a device
    // synchronisation and the whole graph uploaded again (1.2 ms of a 19 ms marginalisation of the 100k-pose graph)
    if (g->cap < g->used * 5 / 2 + (1 << 16)) if (int rc = arena_ensure(g, g->used * 3 + (1 << 20))) return rc;
    if (int rc = sync_device(g)) return rc;
    g->active = true;
    for (int i = 0; i < spg_graph::NB; i++) { g->bt[i].round_open = false; g->bt[i].slot = i; }
    g->B = &g->bt[0];
    g->round_no = 0;
    g->launch_seq = 0;
    g->pipelined = false;
    g->stats = spg_marg_stats{};
    g->log.clear();
    return 0;
}

extern "C" int spg_graph_set_shard_threshold(spg_graph *g, int min_blankets) {
    if (!g) return SPG_EINVAL;
    g->shard_threshold = min_blankets < 0 ? -1 : min_blankets;
    return 0;
}

// Sharding policy for one batch of mutually independent blankets (all ranks evaluate it on identical data, so
// they agree). Model, per GPU: a blanket of n = d*k target variables is one dependent chain of
//     t_b = T24 * max(1, n/24)^2.5     (T24 = 45 us: measured chain of a 24 x 24 blanket)
// and `cap` of them are resident at a time (LDS carve-up: floor(160 KB / tiles) workgroups per CU, at most 6, on
// 256 CUs; blankets whose tiles live in the L2 workspace: one per CU), so a batch takes
//     t_local = max(max_b t_b, sum_b t_b / cap_b),
// and sharded over nr ranks  t_shard = max(max_b t_b, sum_b t_b / (nr cap_b)) + T_x + bytes / BW_x
// with one all-gather of T_x = 30 us (small-message RCCL latency over xGMI) and BW_x = 100 GB/s towards each rank.
// Sharding pays iff t_shard < t_local: wide batches of many blankets; narrow ones (a few hundred blankets finish in
// one chain latency however they are split) are computed redundantly by every rank.
static bool shard_pays(const spg_graph *g, const Batch &bt) {
    const int B = (int)bt.rb.size(), nr = g->nranks;
    if (nr <= 1 || B == 0) return false;
    if (g->shard_threshold >= 0) return B >= g->shard_threshold;
    const int d = g->d;
    double t_sum = 0, t_max = 0, bytes = 0;
    for (const RoundBlanket &r : bt.rb) {
        const double n = (double)d * (r.nv - r.n_remove), nm = (double)d * r.n_remove;
        const double tb = 45e-6 * std::pow(std::max(1.0, n / 24.0), 2.5);
        const double lds = 8.0 * (3 * n * n + nm * nm + nm * n) + 4096.0;
        const double per_cu = lds > 160.0 * 1024 ? 1.0 : std::min(6.0, std::floor(160.0 * 1024 / lds));
        t_sum += tb / (256.0 * per_cu);
        t_max = std::max(t_max, tb);
        int32_t nn, nvv; int64_t nl;
        new_edge_budget(g->opts, d, r.nv - r.n_remove, nn, nvv, nl);
        bytes += 8.0 * (double)(SPG_OUT_LEN(nn, nvv) + nl);
    }
    const double t_local = std::max(t_max, t_sum);
    const double t_shard = std::max(t_max, t_sum / nr) + 30e-6 + bytes / 100e9;
    return t_shard < t_local;
}

// ---- preparing a batch: two steps --------------------------------------------------------------------------------
// (1) layout_region, graph thread (needs g->used / the arena): the out region of the blankets selected into bt. Decides
//     the sharding, cuts the batch into per-rank slices and gives every blanket its out record (the `hdr` part of its
//     rank's chunk) and its new-edge slots (the `body` part): the output side of RoundBlanket::desc, which is all the
//     commit reads. Grows the arena if it has to, opens the round.
//     Returns 1 = laid out, 0 = empty batch, 2 = the arena has to grow first and another batch is running (it writes
//     into the arena): the driver commits that one, then calls again; < 0 error.
// (2) fill_descriptors, either thread (the pipelined driver's submission thread, SPG_HOST_THREADS=2): the descriptors.
static int layout_region(spg_graph *g, Batch &bt, double t0, bool mirror_to_cap) {
    const int B = (int)bt.rb.size();
    if (B == 0) { g->stats.host_seconds += now_s() - t0; return 0; }
    const spg_options &o = g->opts;
    // small rounds are latency-bound: every rank computes them whole, nothing is exchanged
    const bool sharded = shard_pays(g, bt);
    bt.eff_ranks = sharded ? g->nranks : 1;
    bt.eff_rank = sharded ? g->rank : 0;
    const int d = g->d, nr = bt.eff_ranks;
    // ---- contiguous, cost-balanced slices (cost ~ n^3 + E d^3)
    std::vector<double> &cost = g->s_cost;
    cost.assign(B, 0.0);
    double total = 0;
    for (int b = 0; b < B; b++) {
        RoundBlanket &r = bt.rb[b];
        double nn = (double)d * (r.nv - r.n_remove);
        cost[b] = nn * nn * nn + (double)r.ne * d * d * d + 1.0;
        total += cost[b];
    }
    std::vector<int> &first = g->s_first;
    first.assign(nr + 1, B);
    {
        double acc = 0;
        int q = 0;
        first[0] = 0;
        for (int b = 0; b < B; b++) {
            while (q + 1 < nr && acc >= total * (q + 1) / nr) first[++q] = b;
            acc += cost[b];
        }
        for (int qq = q + 1; qq <= nr; qq++) first[qq] = B;
        first[nr] = B;
    }
    // ---- per rank: out records, then new-edge slots
    bt.chunk_hdr.assign(nr, 0);
    int64_t clen = 0;
    for (int q = 0; q < nr; q++) {
        int64_t hdr = 0, body = 0;
        for (int b = first[q]; b < first[q + 1]; b++) {
            RoundBlanket &r = bt.rb[b];
            spg_blanket_desc &bd = r.desc;
            r.rank = q;
            new_edge_budget(o, d, r.nv - r.n_remove, bd.n_new_max, bd.n_new_vert_max, bd.new_len);
            bd.out_off = hdr;  // relative for now
            hdr += SPG_OUT_LEN(bd.n_new_max, bd.n_new_vert_max);
            bd.new_off = body;
            body += bd.new_len;
        }
        bt.chunk_hdr[q] = hdr;
        clen = std::max(clen, hdr + body);
    }
    clen = align_up(std::max<int64_t>(clen, 1), 32);
    int64_t region = align_up(g->used, 32);
    int64_t need = region + clen * nr;
    if (need > g->cap) {
        // grow: pull device-only ranges into the mirror, re-allocate, push the whole mirror back.
        // Not while another batch is running (it writes into the arena): tell the driver to commit it first.
        for (int bi = 0; bi < spg_graph::NB; bi++) if (&g->bt[bi] != &bt && g->bt[bi].round_open) return 2;
        if (int rc = arena_ensure(g, need + need / 2)) return rc;
        if (int rc = sync_device(g)) return rc;
    }
    for (int q = 0; q < nr; q++) {
        int64_t base = region + clen * q;
        for (int b = first[q]; b < first[q + 1]; b++) {
            bt.rb[b].desc.out_off += base;
            bt.rb[b].desc.new_off += base + bt.chunk_hdr[q];
        }
    }
    // mirror_to_cap: the graph thread copies out records into the mirror while the submission thread works: grow it
    // generously here, never under a commit (HostMirror::resize may move the block; only this thread touches it)
    if ((int64_t)g->host.size() < need) g->host.resize((size_t)(mirror_to_cap ? std::max<int64_t>(need, g->cap) : need));
    g->used = need;
    g->dev_synced = need;  // the region is produced on the device
    bt.rinfo.n_blankets = B;
    bt.rinfo.my_first = first[bt.eff_rank];
    bt.rinfo.my_count = first[bt.eff_rank + 1] - first[bt.eff_rank];
    bt.rinfo.region_off = region;
    bt.rinfo.chunk_len = clen;
    bt.rinfo.exchange = sharded ? 1 : 0;
    bt.rinfo.pad_ = 0;
    bt.round_open = true;
    g->stats.n_batches++;
    g->round_no++;
    bt.round_no = g->round_no;
    bt.seq = g->launch_seq++;
    g->stats.host_seconds += now_s() - t0;
    return 1;
}

// (bt.rb is only read: the commit owns it, and on the submission thread a commit may be running)
static void fill_descriptors(spg_graph *g, Batch &bt) {
    const int B = (int)bt.rb.size();
    bt.h_blk.resize(B);
    bt.h_vpo.clear(); bt.h_er.clear(); bt.h_ev.clear();
    if (g->lidx.size() < g->vid.size()) g->lidx.resize(g->vid.size(), -1);
    for (int b = 0; b < B; b++) {
        const RoundBlanket &r = bt.rb[b];
        spg_blanket_desc &bd = bt.h_blk[b];
        append_blanket_desc(g, bt.rb_verts.data() + r.vbeg, r.nv, r.n_remove, bt.rb_edges.data() + r.ebeg, r.ne, bd, bt.h_vpo, bt.h_er, bt.h_ev);
        bd.n_new_max = r.desc.n_new_max; bd.n_new_vert_max = r.desc.n_new_vert_max;
        bd.new_off = r.desc.new_off; bd.new_len = r.desc.new_len; bd.out_off = r.desc.out_off;
    }
}

// both steps for the blankets already selected into *g->B
static int prepare_scheduled(spg_graph *g, spg_round_info *info, double t0) {
    Batch &bt = *g->B;
    const int rc = layout_region(g, bt, t0, false);
    if (rc != 1) return rc;
    const double t1 = now_s();
    fill_descriptors(g, bt);
    if (info) *info = bt.rinfo;
    g->stats.host_seconds += now_s() - t1;
    return 1;
}

extern "C" int spg_graph_round_prepare(spg_graph *g, spg_round_info *info) {
    if (!g || !g->active) return SPG_ESTATE;
    Batch &bt = *g->B;
    if (bt.round_open) return SPG_ESTATE;
    double t0 = now_s();
    schedule_round(g);
    g->stats.schedule_seconds += now_s() - t0;
    return prepare_scheduled(g, info, t0);
}

static int harvest_kld(spg_graph *g, Batch &bt);
// where the mailbox of a batch starts in the arena's offsets: the chunk of the rank that computes it
static inline int64_t mail_base(const Batch &bt) { return bt.rinfo.region_off + bt.rinfo.chunk_len * bt.eff_rank; }
// graph-thread half of spg_graph_round_compute: launch tag, late results of the slot's previous launch
static int compute_prologue(spg_graph *g, Batch &bt) {
    bt.tag = ++g->ctx->tag_counter;
    return harvest_kld(g, bt);
}
// submission-thread half: the round descriptor and the hand-over to the backend
static int compute_submit(spg_graph *g, Batch &bt) {
    spg_round_desc rd{};
    rd.opts = &g->opts;
    rd.n_blankets = bt.rinfo.n_blankets;
    rd.first = bt.rinfo.my_first;
    rd.count = bt.rinfo.my_count;
    rd.blankets = bt.h_blk.data();
    rd.vert_pose_off = bt.h_vpo.data();
    rd.edges = bt.h_er.data();
    rd.edge_vert = bt.h_ev.data();
    rd.n_vert_total = (int64_t)bt.h_vpo.size();
    rd.n_edge_total = (int64_t)bt.h_er.size();
    rd.n_edge_vert_total = (int64_t)bt.h_ev.size();
    rd.mail_base = mail_base(bt);
    rd.mail_len = (bt.eff_ranks == 1 && g->ctx->be.mailbox) ? bt.chunk_hdr[bt.eff_rank] : 0;
    rd.slot = g->pipelined ? bt.slot : 0;
    rd.tag = bt.tag;
    bt.used_mailbox = rd.mail_len > 0;
    bt.t_launch = now_s();
    return g->ctx->be.run_round(g->ctx->be.user, g->dev, &rd);
}

static void submission_main(spg_graph *g) {
    uint32_t idle = 0;
    while (g->sub.run.load(std::memory_order_acquire)) {
        const uint32_t h = g->sub.head.load(std::memory_order_relaxed);
        if (h == g->sub.tail.load(std::memory_order_acquire)) { spin_wait(idle); continue; }
        idle = 0;
        Batch *b = g->sub.q[h % spg_graph::SUBQ];
        const double t0 = now_s();
        fill_descriptors(g, *b);
        b->submit_rc = compute_submit(g, *b);
        g->sub.seconds += now_s() - t0;
        g->sub.head.store(h + 1, std::memory_order_release);
        b->submitted.store(1, std::memory_order_release);
    }
}
static void submission_start(spg_graph *g) {
    if (g->sub_active) return;
    g->sub.head.store(0); g->sub.tail.store(0);
    g->sub.seconds = 0;
    g->sub.run.store(true, std::memory_order_release);
    g->sub_thread = std::thread(submission_main, g);
    g->sub_active = true;
#if defined(__linux__)
    // keep the two threads on neighbouring cores (same L3): the lists one writes and the other reads then move
    // through the shared cache instead of across the socket. Best effort; only CPUs this process may use.
    static const bool pin = [] { const char *e = getenv("SPG_PIN_THREADS"); return !(e && e[0] == '0'); }();
    if (pin) {
        int cpu = sched_getcpu();
        cpu_set_t allowed;
        if (cpu >= 0 && sched_getaffinity(0, sizeof allowed, &allowed) == 0) {
            for (int cand : {cpu ^ 1, cpu + 1, cpu - 1}) {
                if (cand >= 0 && cand < CPU_SETSIZE && cand != cpu && CPU_ISSET(cand, &allowed)) {
                    cpu_set_t one;
                    CPU_ZERO(&one); CPU_SET(cand, &one);
                    (void)pthread_setaffinity_np(g->sub_thread.native_handle(), sizeof one, &one);
                    break;
                }
            }
        }
    }
#endif
}
static void wait_submitted(Batch &b) {
    uint32_t spins = 0;
    while (!b.submitted.load(std::memory_order_acquire)) spin_wait(spins);
}
void quiesce_submission(spg_graph *g) {
    for (int i = 0; i < spg_graph::NB; i++) wait_submitted(g->bt[i]);
}
static void submission_stop(spg_graph *g) {
    if (!g->sub_active) return;
    quiesce_submission(g);
    g->sub.run.store(false, std::memory_order_release);
    g->sub_thread.join();
    g->sub_active = false;
    g->stats.launch_seconds += g->sub.seconds;   // (the thread's time is reported as launch_seconds)
}
static void submission_push(spg_graph *g, Batch &b) {
    b.submitted.store(0, std::memory_order_relaxed);
    b.submit_rc = 0;
    const uint32_t t = g->sub.tail.load(std::memory_order_relaxed);
    g->sub.q[t % spg_graph::SUBQ] = &b;
    g->sub.tail.store(t + 1, std::memory_order_release);
}

// Late results of a batch that was committed by polling: once its launch has completed, pick up the
// per-blanket KLD (and a possible SPG_ST_KLD_NOT_PD) from the mailbox — the NFR value, or the GLC one under SPG_FLAG_GLC_KLD.
static int harvest_kld(spg_graph *g, Batch &bt) {
    if (bt.kld_pending.empty()) return 0;
    const bool slotted = g->ctx->be.synchronize_slot && g->ctx->be.mailbox_slot;
    int rc = slotted ? g->ctx->be.synchronize_slot(g->ctx->be.user, bt.slot) : g->ctx->be.synchronize(g->ctx->be.user);
    if (rc) return rc;
    const double *mail = slotted ? g->ctx->be.mailbox_slot(g->ctx->be.user, bt.slot) : g->ctx->be.mailbox(g->ctx->be.user);
    for (auto &pr : bt.kld_pending) {
        const double *rec = mail + pr.second;
        BlanketLog &lg = g->log[pr.first];
        lg.kld = rec[2];
        lg.min_gap = rec[3];
        lg.status = (int32_t)rec[0];
        lg.info = (int32_t)rec[1];   // (SPG_INFO_GLC_KLD_SKIPPED is decided in the tail, after the ready word)
        if (std::isfinite(rec[2])) g->stats.kld_sum += rec[2];
    }
    bt.kld_pending.clear();
    return 0;
}

extern "C" int spg_graph_round_compute(spg_graph *g) {
    if (!g || !g->active) return SPG_ESTATE;
    Batch &bt = *g->B;
    if (!bt.round_open) return SPG_ESTATE;
    double t0 = now_s();
    // the mailbox of this slot is about to be rewritten: collect what the previous launch left in it
    if (int hrc = compute_prologue(g, bt)) return hrc;
    int rc = compute_submit(g, bt);
    g->stats.device_seconds += now_s() - t0;
    g->stats.launch_seconds += now_s() - t0;
    if (rc && g->ctx->is_hip) copy_backend_error(g->ctx);
    return rc;
}

extern "C" int spg_graph_round_commit(spg_graph *g) {
    if (!g || !g->active) return SPG_ESTATE;
    Batch &bt = *g->B;
    if (!bt.round_open) return SPG_ESTATE;
    double t0 = now_s();
    wait_submitted(bt);   // (pipelined driver: the submission thread may still be handing the batch over)
    if (bt.submit_rc) {
        if (g->ctx->is_hip) copy_backend_error(g->ctx);
        return bt.submit_rc;
    }
    const int nr = bt.eff_ranks;
    const bool slotted = g->pipelined && g->ctx->be.synchronize_slot && g->ctx->be.mailbox_slot;
    const double *mail = nullptr;
    if (bt.used_mailbox && g->ctx->be.mailbox)
        mail = slotted ? g->ctx->be.mailbox_slot(g->ctx->be.user, bt.slot) : g->ctx->be.mailbox(g->ctx->be.user);
    int rc = 0;
    bool polled = false;
    if (mail && nr == 1) {
        // Poll the ready tags the kernel writes (system-scope release) after each blanket's graph-update
        // data is complete; the launch itself may still be finishing KLD tails. Bounded spin: after
        // ~5 s fall back to a stream synchronisation, which also surfaces a faulted kernel.
        const int64_t base = mail_base(bt);
        const double t_spin = now_s();
        // (SPG_POLL_SPIN_S: tests set 0 to force the synchronisation path on ordinary batches)
        const char *sl_env = getenv("SPG_POLL_SPIN_S");
        const double spin_limit = sl_env ? atof(sl_env) : 5.0;
        polled = true;
        bool first_seen = false;
        for (const RoundBlanket &r : bt.rb) {
            const volatile double *flag = mail + (r.desc.out_off - base) + 5;
            if (first_seen == false && &r != &bt.rb[0]) { g->tr_first += now_s() - bt.t_launch; first_seen = true; }
            uint32_t spins = 0;
            while (mail_state(*flag, bt.tag) == MAIL_NOT_YET) {
                if ((++spins & 0x3fff) == 0 && now_s() - t_spin > spin_limit) { polled = false; break; }
                cpu_pause();
            }
            if (!polled) break;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!polled) {
        rc = slotted ? g->ctx->be.synchronize_slot(g->ctx->be.user, bt.slot) : g->ctx->be.synchronize(g->ctx->be.user);
        if (rc) return rc;
        if (mail && nr == 1) {
            // the launch has completed: every record must carry this launch's tag now. One that does not was never written
            // (a blanket no kernel took, a kernel that died): an error, never a graph update from whatever the cell held.
            const int64_t base = mail_base(bt);
            for (const RoundBlanket &r : bt.rb) {
                if (mail_state(mail[(r.desc.out_off - base) + 5], bt.tag) == MAIL_NOT_YET)
                    return set_err(g->ctx, SPG_EHIP, "the blanket of vertex %s did not deliver its out record although its launch has completed", std::to_string(g->vid[r.root]).c_str());
            }
        }
    }
    g->tr_n++; g->tr_wait += now_s() - t0; g->tr_age += t0 - bt.t_launch;
    // read back the out-record part of every rank chunk (mailbox: already in host memory)
    for (int q = 0; q < nr; q++) {
        if (bt.chunk_hdr[q] == 0) continue;
        int64_t base = bt.rinfo.region_off + bt.rinfo.chunk_len * q;
        if (mail && q == bt.eff_rank) { memcpy(g->host.data() + base, mail, (size_t)bt.chunk_hdr[q] * 8); continue; }
        rc = g->ctx->be.download(g->ctx->be.user, g->host.data() + base, (char *)g->dev + base * 8, bt.chunk_hdr[q]);
        if (rc) return rc;
    }
    double t1 = now_s();
    g->stats.device_seconds += t1 - t0;
    // the payload part of the region stays device-only until someone asks for it
    mark_stale(g, bt.rinfo.region_off, bt.rinfo.region_off + bt.rinfo.chunk_len * nr);
    // updateInputGraph (src/vertex_remover.cpp:500-546), in list order
    std::vector<int32_t> &vix = g->s_vix;
    for (size_t b = 0; b < bt.rb.size(); b++) {
        RoundBlanket &r = bt.rb[b];
        const spg_blanket_desc &bd = r.desc;
        const double *rec = g->host.data() + bd.out_off;
        int status = (int)rec[0], inf = (int)rec[1], n_new = (int)rec[4];
        PT0;
        g->log.push_back({g->vid[r.root], bt.round_no, status, inf, rec[2], rec[3]});
        if (polled && (status == SPG_OK)) bt.kld_pending.push_back({(int32_t)g->log.size() - 1, bd.out_off - mail_base(bt)});
        g->stats.max_blanket = std::max(g->stats.max_blanket, r.nv);
        const int32_t *rverts = bt.rb_verts.data() + r.vbeg;
        const int32_t *redges = bt.rb_edges.data() + r.ebeg;
        bool fine = (status == SPG_OK || status == SPG_ST_KLD_NOT_PD);
        if (!fine) { g->stats.n_bad_status++; continue; }
        if (!polled && std::isfinite(rec[2])) g->stats.kld_sum += rec[2];
        PT(7);
        for (int ei_ = 0; ei_ < r.ne; ei_++) retire_edge(g, redges[ei_]);
        PT(8);
        for (int i = 0; i < r.n_remove; i++) {
            int32_t v = rverts[i];
            g->valive[v] = 0;
            g->vr[v].adj.clear();
            g->n_live_v--;
            g->stats.n_removed++;
        }
        PT(9);
        if (!out_record_well_formed(rec, bd, r.nv)) {
            char msg[256];
            snprintf(msg, sizeof msg, "out record of the blanket of vertex %d is not well formed (status %d, %d new edges of at most %d, k + m = %d, m = %d; words %g %g %g %g %g %g | %g %g %g %g)", g->vid[r.root], status, n_new, bd.n_new_max, r.nv, r.n_remove,
                     rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7], rec[8], rec[9]);
            return set_err(g->ctx, SPG_EHIP, "%s", msg);
        }
        const int64_t key0 = g->key_base + (int64_t)g->lpos[r.root] * spg_graph::kKeyStride;
        for_each_new_edge(rec, n_new, bd.n_new_max, [&](int e, int kind, int64_t rel, int32_t len, int nv, const double *lv) {
            vix.resize(nv);
            for (int i = 0; i < nv; i++) vix[i] = rverts[(int)lv[i]];
            add_edge_idx(g, kind, nv, vix.data(), bd.new_off + rel, len, key0 + e);
            g->stats.n_new_edges++;
        });
        PT(10);
    }
    bt.round_open = false;
    release_batch_owners(g, bt);
    g->stats.n_rounds = g->round_no;
    g->stats.host_seconds += now_s() - t1;
    g->stats.commit_seconds += now_s() - t1;
    return 0;
}

extern "C" int spg_graph_marginalize_end(spg_graph *g, spg_marg_stats *stats) {
    if (!g || !g->active) return SPG_ESTATE;
    submission_stop(g);
    g->active = false;
    for (int i = 0; i < spg_graph::NB; i++) (void)harvest_kld(g, g->bt[i]);
    for (int i = 0; i < spg_graph::NB; i++) { g->bt[i].round_open = false; release_batch_owners(g, g->bt[i]); g->bt[i].rb.clear(); }
    for (int32_t oid : g->transient) owner_release(g, oid);
    g->transient.clear();
    g->B = &g->bt[0];
    if (g->ctx->is_hip) (void)spg::hip_backend_end_of_call(&g->ctx->be);
    if (g->tr_n && getenv("SPG_TRACE"))
        fprintf(stderr, "spg trace: %ld batches; per batch: launch call -> commit start %.1f us, wait for the ready words %.1f us (launch call -> first blanket ready %.1f us)\n",
                g->tr_n, 1e6 * g->tr_age / g->tr_n, 1e6 * g->tr_wait / g->tr_n, 1e6 * g->tr_first / g->tr_n);
    g->tr_n = 0; g->tr_age = g->tr_wait = g->tr_first = 0;
    if (g->ctx->is_hip) g->stats.n_launches = spg::hip_backend_launches(&g->ctx->be);
#ifdef SPG_SCHED_PROF
    if (getenv("SPG_SCHED_PROF")) {
        const char *nm[12] = {"neighbourhood", "owner scan", "select:reg", "defer", "-", "select:sort", "select:edges", "commit:log", "commit:rm edges", "commit:rm verts", "commit:add", "prepare"};
        for (int i = 0; i < 12; i++) { fprintf(stderr, "sched %-14s %10llu calls %8.3f Mcycles\n", nm[i], prof_n[i], prof_t[i] * 1e-6); prof_t[i] = prof_n[i] = 0; }
    }
#endif
    if (stats) *stats = g->stats;
    return g->stats.n_bad_status ? SPG_EBLANKET : 0;
}

// the batch in flight that was launched first, or nullptr
static Batch *oldest_open_batch(spg_graph *g) {
    Batch *o = nullptr;
    for (int i = 0; i < spg_graph::NB; i++) if (g->bt[i].round_open && (!o || g->bt[i].seq < o->seq)) o = &g->bt[i];
    return o;
}

// Move blankets [from, to) of a freshly scheduled batch into another (idle) batch: all of them are
// mutually independent, so the parts can be launched back to back on different slots.
static void move_blankets(spg_graph *g, Batch &a, size_t from, size_t to, Batch &b) {
    b.rb.clear(); b.rb_verts.clear(); b.rb_edges.clear();
    const int32_t bidx = (int32_t)(&b - g->bt);
    for (size_t i = from; i < to; i++) {
        RoundBlanket r = a.rb[i];
        int32_t vb = (int32_t)b.rb_verts.size(), eb = (int32_t)b.rb_edges.size();
        b.rb_verts.insert(b.rb_verts.end(), a.rb_verts.begin() + r.vbeg, a.rb_verts.begin() + r.vbeg + r.nv);
        b.rb_edges.insert(b.rb_edges.end(), a.rb_edges.begin() + r.ebeg, a.rb_edges.begin() + r.ebeg + r.ne);
        r.vbeg = vb; r.ebeg = eb;
        if (r.owner >= 0) { g->owners[r.owner].batch = bidx; g->owners[r.owner].off = vb; }
        b.rb.push_back(r);
    }
}

extern "C" int spg_graph_marginalize(spg_graph *g, const int32_t *which, int n, const spg_options *opts, spg_marg_stats *stats) {
    return spg_graph_marginalize_ranks(g, which, n, opts, 0, 1, nullptr, nullptr, stats);
}

extern "C" int spg_graph_marginalize_ranks(spg_graph *g, const int32_t *which, int n, const spg_options *opts, int rank, int nranks,
                                           spg_exchange_fn exchange, void *exchange_user, spg_marg_stats *stats) {
    if (!g) return SPG_EINVAL;
    // no callback: the built-in RCCL all-gather of the context (spg_ctx_create_ranks with the same rank / nranks)
    const bool builtin = nranks > 1 && !exchange;
    if (builtin && (!g->ctx->rccl || g->ctx->nranks != nranks || g->ctx->rank != rank))
        return set_err(g->ctx, SPG_EINVAL, "spg_graph_marginalize_ranks: no exchange callback and the context has no matching RCCL communicator (spg_ctx_create_ranks)");
    int launches0 = (g && g->ctx->is_hip) ? spg::hip_backend_launches(&g->ctx->be) : 0;
    const double t_call = now_s();
    int rc = spg_graph_marginalize_begin(g, which, n, opts, rank, nranks);
    if (rc) return rc;
    const double t_begun = now_s();
    const char *env = getenv("SPG_NO_PIPELINE");
    g->pipelined = g->ctx->be.synchronize_slot && g->ctx->be.mailbox_slot && !(env && env[0] == '1');
    // single rank, NFR Tree at the stored estimates: blanket by blanket through the persistent worker (streaming driver);
    // whatever it leaves (rc 1: blankets the worker does not take) goes through the batch driver below
    int stream_rc = 1;
    if (nranks == 1 && !exchange) stream_rc = stream_marginalize(g);
    else if (nranks > 1) {
        // Several ranks, one replicated graph. A batch is worth sharding + one all-gather only when it is wide (shard_pays);
        // lists whose batches are narrow — the 100k-pose lattice: ~200 independent blankets at a time — are computed whole by
        // every rank with nothing exchanged, and then nothing ties the ranks to the same batches either: each rank may run
        // its own streaming driver. Results do not depend on the schedule (blanket edges are summed in key order), so the
        // replicas stay equal in content; their arena LAYOUTS diverge (records are placed in launch order), and regions are
        // exchanged by offset — so a graph that has streamed on several ranks never shards again (layout_diverged).
        // The decision is taken on the first pass of the batch scheduler, identically on every rank.
        bool independent = g->layout_diverged;
        if (!independent && g->shard_threshold < 0) {
            const std::vector<int32_t> saved = g->pending;
            g->B = &g->bt[0];
            schedule_round(g);
            independent = !g->bt[0].rb.empty() && !shard_pays(g, g->bt[0]);
            release_batch_owners(g, g->bt[0]);
            g->bt[0].rb.clear(); g->bt[0].rb_verts.clear(); g->bt[0].rb_edges.clear();
            for (int32_t oid : g->transient) owner_release(g, oid);
            g->transient.clear();
            g->pending = saved;
            g->pend_head = 0;
        }
        if (independent) {
            const int rank0 = g->rank, nranks0 = g->nranks;
            g->rank = 0; g->nranks = 1;
            bool started = false;
            stream_rc = stream_marginalize(g, &started);
            if (started || g->layout_diverged) g->layout_diverged = true;   // (and the batch driver below, if it gets the rest, runs without sharding)
            else { g->rank = rank0; g->nranks = nranks0; }
        }
    }
    if (stream_rc <= 0) {
        const double t_streamed = now_s();
        int rc2 = spg_graph_marginalize_end(g, stats);
        if (getenv("SPG_TRACE")) fprintf(stderr, "spg trace: marginalize: begin %.3f ms, stream %.3f ms, end %.3f ms\n", 1e3 * (t_begun - t_call), 1e3 * (t_streamed - t_begun), 1e3 * (now_s() - t_streamed));
        if (stats && g->ctx->is_hip) stats->n_launches -= launches0;
        return stream_rc < 0 ? stream_rc : rc2;
    }
    auto do_exchange = [&](Batch &b) -> int {
        if (!b.rinfo.exchange) return 0;
        double tx = now_s();
        int erc = g->ctx->be.synchronize(g->ctx->be.user);  // this rank's chunk is complete in memory
        if (erc) return erc;
        erc = builtin ? spg_allgather_region(g->ctx, g->dev, b.rinfo.region_off, b.rinfo.chunk_len)
                      : exchange(exchange_user, g->dev, b.rinfo.region_off, b.rinfo.chunk_len, g->nranks, g->rank);
        g->stats.n_exchanged++;
        g->stats.exchanged_bytes += 8.0 * (double)b.rinfo.chunk_len * g->nranks;
        g->stats.exchange_seconds += now_s() - tx;
        return erc;
    };
    if (!g->pipelined) {
        for (;;) {
            rc = spg_graph_round_prepare(g, nullptr);
            if (rc <= 0) break;
            if ((rc = spg_graph_round_compute(g)) != 0) break;
            if ((rc = do_exchange(*g->B)) != 0) break;
            if ((rc = spg_graph_round_commit(g)) != 0) break;
        }
    } else {
        // Up to NB batches in flight. After every commit one scheduling pass picks whatever commutes
        // with the batches still running (and with everything earlier in the list); a large pick is
        // cut into as many parts as there are idle slots so that the host work of one part overlaps the
        // device work of the others. With nothing schedulable, wait for the oldest batch and apply it.
        constexpr int NB = spg_graph::NB;
        rc = 0;
        const char *e1 = getenv("SPG_SPLIT_MIN"), *e2 = getenv("SPG_MAX_INFLIGHT");
        // defaults from sweeps on 100k-pose lattices with rings of 250 ... 1000: parts of >= 48 blankets,
        // four batches in flight (more only add passes), patience 16
        const size_t split_min = e1 ? (size_t)atoi(e1) : 48;
        const int max_inflight = e2 ? std::max(1, std::min(NB, atoi(e2))) : 4;
        auto commit_all = [&]() -> int {
            while (Batch *o = oldest_open_batch(g)) {
                g->B = o;
                if (int c = spg_graph_round_commit(g)) return c;
            }
            return 0;
        };
        // SPG_HOST_THREADS=2: descriptors + device hand-over on a second host thread. Off by default: measured on the
        // bench workload it does not pay (33.1 vs 31.9 ms per step with the two threads on neighbouring cores, 48 ms
        // on different L3s) — a batch waits for its round trip through the device, not for the graph thread.
        static const bool use_thread = [] { const char *e = getenv("SPG_HOST_THREADS"); return e && e[0] == '2'; }();
        auto launch_batch = [&](Batch &b, double t0) -> int {
            g->B = &b;
            // threaded: descriptors + hand-over on the submission thread; region, tag and late results here
            const bool threaded = use_thread && !shard_pays(g, b);
            auto prepare = [&](double t) { return threaded ? layout_region(g, b, t, true) : prepare_scheduled(g, nullptr, t); };
            int prc = prepare(t0);
            if (prc == 2) {  // the arena has to grow: nothing may be running while it is re-allocated
                if (int c = commit_all()) return c;
                g->B = &b;
                prc = prepare(now_s());
            }
            if (prc <= 0) return prc;
            if (!threaded) return spg_graph_round_compute(g);
            if (int hrc = compute_prologue(g, b)) return hrc;
            submission_start(g);
            submission_push(g, b);
            return 0;
        };
        for (;;) {
            bool launched = false;
            int f = -1, nfree = 0;
            for (int i = 0; i < NB; i++) if (!g->bt[i].round_open) { if (f < 0) f = i; nfree++; }
            nfree -= NB - max_inflight;
            if (nfree <= 0) f = -1;
            if (f >= 0 && g->pend_head < g->pending.size()) {
                Batch &bt = g->bt[f];
                g->B = &bt;
                double t0 = now_s();
                schedule_round(g);
                g->stats.schedule_seconds += now_s() - t0;
                if (bt.rb.empty()) {
                    g->stats.host_seconds += now_s() - t0;
                } else if (shard_pays(g, bt)) {
                    // a wide batch: worth sharding over the ranks. Finish what is in flight, then run it
                    // as one exchanged round (compute own slice, all-gather, commit).
                    if ((rc = commit_all()) != 0) break;
                    if ((rc = launch_batch(bt, t0)) != 0) break;
                    if ((rc = do_exchange(bt)) != 0) break;
                    g->B = &bt;
                    if ((rc = spg_graph_round_commit(g)) != 0) break;
                    continue;
                } else {
                    size_t S = bt.rb.size();
                    int parts = (int)std::min<size_t>((size_t)nfree, std::max<size_t>(1, S / split_min));
                    // hand parts 1..parts-1 to other idle batches, keep part 0 here
                    std::vector<Batch *> tgt;
                    for (int i = 0; i < NB && (int)tgt.size() < parts - 1; i++) if (i != f && !g->bt[i].round_open) tgt.push_back(&g->bt[i]);
                    parts = (int)tgt.size() + 1;
                    size_t per = (S + parts - 1) / parts;
                    for (int pi = 1; pi < parts; pi++) move_blankets(g, bt, std::min(S, per * pi), std::min(S, per * (pi + 1)), *tgt[pi - 1]);
                    bt.rb.resize(std::min(S, per));
                    if ((rc = launch_batch(bt, t0)) != 0) break;
                    for (int pi = 1; pi < parts && rc == 0; pi++) if (!tgt[pi - 1]->rb.empty()) rc = launch_batch(*tgt[pi - 1], now_s());
                    if (rc != 0) break;
                    launched = true;
                }
            }
            Batch *oldest = oldest_open_batch(g);
            if (!oldest) {
                if (!launched) break;  // nothing in flight, nothing schedulable: done
                continue;
            }
            g->B = oldest;
            if ((rc = spg_graph_round_commit(g)) != 0) break;
        }
        // drain on error
        quiesce_submission(g);
        for (int s_ = 0; s_ < spg_graph::NB; s_++) if (g->bt[s_].round_open) { g->ctx->be.synchronize(g->ctx->be.user); g->bt[s_].round_open = false; }
        g->B = &g->bt[0];
    }
    int rc2 = spg_graph_marginalize_end(g, stats);
    if (stats && g->ctx->is_hip) stats->n_launches -= launches0;
    return rc < 0 ? rc : rc2;
}
