// csrc/spg_hip_backend.cpp — the HIP backend: launches one conflict-free round of blankets (or hands it to the
// persistent worker), owns the launch slots and their buffers, and opens the worker's queue to the streaming driver.
// Host-only code: what goes where is decided in spg_round_plan.hpp, the kernels are reached through the launch entry
// points of spg_kernels.hip, spg_nfr_ip.hip and spg_dense.hip.
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include "../../include/spg.h"
#include "spg_blanket_layout.hpp"
#include "spg_hip_buffers.hpp"
#include "spg_internal.h"
#include "spg_round_plan.hpp"

namespace spg {

// (`err` is HipBackend::err, 512 bytes, as the member array or through a char * alias)
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { snprintf(err, (size_t)512, "%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); return SPG_EHIP; } } while (0)

namespace {

bool env_is(const char *name, char c) { const char *e = getenv(name); return e && e[0] == c; }

struct HipBackend {
    int device = 0;
    char err[512] = {0};
    struct Timed { hipEvent_t a, b; double bytes; int blankets; };
    // Independent launch slots (stream + descriptor buffers + pinned staging + pinned mailbox +
    // large-blanket workspace) so that the host can prepare and launch one batch of blankets while the
    // previous one is still running.
    struct Slot {
        hipStream_t stream = nullptr;
        DevBuf desc, gws, ipws, lpose, lmeta;
        PinnedBuf mail;                               // pinned host mailbox the kernel writes out records into
        PinnedBuf stage;                              // pinned host staging for the descriptor upload
        bool busy = false;                            // work was queued on the stream since its last synchronisation
        RoundPlan plan;                               // scratch of hip_run_round (the lists keep their capacity)
        // Waiting for a slot goes through the event recorded behind its last kernel: hipStreamSynchronize on
        // a stream that ends in a kernel has to submit a marker first and was measured at ~10 us per call,
        // hipEventSynchronize on an already recorded event at ~1 us.
        hipEvent_t done = nullptr, wait_ev = nullptr;
        DevBuf bar;                                   // fine-grained device memory the host writes through the PCIe BAR
        // blankets of the last batch that went through the persistent worker: addresses of their final words in the
        // pinned mailbox (wait_slot polls them: the slot's buffers may be rewritten once all of them are final)
        std::vector<const volatile double *> finals;
        double final_word = 0;
        DevBuf pkt;                                   // fine-grained device memory for the packets (host writes, BAR)
        bool stream_dirty = false;                    // something was queued on `stream` since the last wait
        std::vector<Timed> pending;
        // per slot, so that a submission thread working on one slot and the graph thread draining
        // another never share state
        std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
        double prof_ms = 0, prof_bytes = 0;
        long long prof_launches = 0, prof_blankets = 0;
    };
    static constexpr int NSLOT = 8;
    Slot slots[NSLOT];
    // the persistent worker kernel (one per backend, alive between the first narrow batch of a marginalisation and
    // the next full synchronisation)
    struct Worker {
        hipStream_t stream = nullptr;
        DevBuf qmem;                                  // fine-grained device memory; the host stores through the BAR
        DevBuf ticket;                                // device memory
        WorkQ *q() const { return (WorkQ *)qmem.p; }
        hipEvent_t ev_a = nullptr, ev_b = nullptr;
        bool running = false, disabled = false;
        int D = 0, alg = 0;
        unsigned long long tail = 0;                  // host copy of q->tail
        double bytes = 0;                             // algorithmic bytes / blankets handed over since it started
        long long blankets = 0;
        int bells = 1, lazy = 0;                     // (more doorbell copies / lazier polls: measured, no effect)
        int wgs = 256;                                // one per CU: launched kernels must always find room next to it
        std::chrono::steady_clock::time_point last_push;
    } worker;
    int batches_in_call = 0;                          // batches since the last full synchronisation
    // streaming driver (hip_stream_open): its own packet ring (fine-grained device memory) and pinned mailbox
    DevBuf st_pkt;
    PinnedBuf st_mail;
    int worker_cooldown = 0;                          // batches to go before the worker is considered again
    double prof_big_ms = 0, prof_big_flops = 0;       // large-blanket dense pipeline (always accumulated)
    long long prof_big_count = 0;
    int prof_big_nmax = 0;
    double prof_worker_ms = 0, prof_worker_bytes = 0;
    long long prof_worker_runs = 0, prof_worker_blankets = 0;
    int lds_limit = 160 * 1024;
    double fd_rel_tol = kFdRelTol;                    // spg_ctx_set_factor_descent, resolved (0: exactly fd_max_cycles cycles)
    int fd_max_cycles = kFdMaxCycles;
    bool large_bar = false;       // the host can store straight into device memory (hipDeviceAttributeIsLargeBar)
    std::atomic<int> n_launches{0};
    // environment switches, read once
    const bool force_one_wave = env_is("SPG_ONE_WAVE", '1');   // never use the two-wavefront latency variant (A/B timing)
    const bool worker_env = !env_is("SPG_WORKER", '0');
    const bool worker_stamp = env_is("SPG_WORKER_STAMP", '1');
    const bool echo_test = env_is("SPG_WORKER_ECHO_TEST", '1');
    const bool force_big = env_is("SPG_FORCE_BIG", '1');       // diagnostic / tests
    const bool bar_ok = !env_is("SPG_BAR_DESC", '0');
    const int mapped_limit = [] { const char *e = getenv("SPG_MAPPED_DESC"); return e ? atoi(e) : 512; }();
    // optional per-launch timing with HIP events on the launch stream (bench.py roofline leg)
    bool profiling = false;
    int prof_stride = 1, prof_tick = 0;   // time every prof_stride-th launch (1 = all)

    int make_current() {   // (a thread-local read; hipSetDevice costs a microsecond per launch)
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != device) HIPCHK(hipSetDevice(device));
        return 0;
    }
    // Growth of the buffers. hipFree / hipHostFree wait for the whole device: the worker must not be spinning on it, and
    // (`idle`) nothing queued on that stream may still read the block.
    int ensure(Slot &S, DevBuf &b, size_t need) {
        if (need <= b.cap) return 0;
        const size_t nc = std::max(need, b.cap * 2);
        if (b.p) { if (int rc = worker_stop()) return rc; HIPCHK(hipStreamSynchronize(S.stream)); HIPCHK(b.release()); }
        HIPCHK(b.alloc(nc));
        return 0;
    }
    // fine-grained memory may be refused: *ok tells, and the caller turns off what needed it
    int ensure_fine(DevBuf &b, size_t need, size_t min_cap, bool *ok) {
        *ok = true;
        if (need <= b.cap) return 0;
        if (int rc = worker_stop()) return rc;
        HIPCHK(b.release());
        if (b.alloc_fine(std::max(need, min_cap)) != hipSuccess) { (void)hipGetLastError(); *ok = false; }
        return 0;
    }
    int ensure_pinned(PinnedBuf &b, size_t need, bool doubling, hipStream_t idle = nullptr) {
        if (need <= b.cap) return 0;
        const size_t nc = doubling ? std::max(need, b.cap * 2) : need;
        if (int rc = worker_stop()) return rc;
        if (b.h && idle) HIPCHK(hipStreamSynchronize(idle));
        HIPCHK(b.release());
        HIPCHK(b.alloc(nc));
        return 0;
    }
    int wait_slot(Slot &S) {
        if (S.wait_ev) { HIPCHK(hipEventSynchronize(S.wait_ev)); S.wait_ev = nullptr; }
        else if (S.stream_dirty) HIPCHK(hipStreamSynchronize(S.stream));
        S.stream_dirty = false;
        if (!S.finals.empty()) {
            const auto t0 = std::chrono::steady_clock::now();
            for (const volatile double *p : S.finals) {
                uint32_t spins = 0;
                while (*p != S.final_word) {
                    if ((++spins & 0xfff) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 10.0) {
                        snprintf(err, sizeof err, "persistent worker: a blanket did not complete within 10 s");
                        return SPG_EHIP;
                    }
#if defined(__x86_64__)
                    __builtin_ia32_pause();
#endif
                }
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            S.finals.clear();
        }
        S.busy = false;
        return 0;
    }
    void drain_profile(Slot &S) {
        for (auto &t : S.pending) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
                S.prof_ms += ms; S.prof_bytes += t.bytes; S.prof_launches++; S.prof_blankets += t.blankets;
            }
            S.pool.push_back({t.a, t.b});
        }
        S.pending.clear();
    }
    int worker_stop();
    int worker_start(int D, int alg);
    int launch_bin(Slot &S, const PlanBin &B, const KArgs &ka);
    // the steps of hip_run_round
    struct Staged { char *base; size_t o_blk, o_vpo, o_er, o_ev, o_list; };
    int push_to_worker(Slot &S, const spg_round_desc *rd, void *arena);
    int stage_descriptors(Slot &S, const spg_round_desc *rd, Staged &st);
    int launch_bins(Slot &S, KArgs &ka, const int32_t *list);
    int local_prepass(Slot &S, const spg_round_desc *rd, void *arena, IpArgs &ia);
    int launch_generic(Slot &S, const spg_round_desc *rd, void *arena, const KArgs &ka, const int32_t *list);
    int run_big_blankets(Slot &S, const spg_round_desc *rd, void *arena, double *mail_dev);
    int run_round(void *arena, const spg_round_desc *rd);
};

// One bin of blankets on the slot's stream. With profiling on, every prof_stride-th launch carries its own pair of events.
int HipBackend::launch_bin(Slot &S, const PlanBin &B, const KArgs &ka) {
    const int nblocks = (int)B.list.size();
    Timed t{};
    const bool timed = profiling && (prof_tick++ % prof_stride == 0);
    if (timed) {
        if (S.pool.empty()) {
            HIPCHK(hipEventCreate(&t.a));
            HIPCHK(hipEventCreate(&t.b));
        } else { t.a = S.pool.back().first; t.b = S.pool.back().second; S.pool.pop_back(); }
        t.bytes = B.bytes; t.blankets = nblocks;
    }
    const hipEvent_t stop = timed ? t.b : S.done;
    if (int rc = hip_blanket_launch(B.variant, S.stream, timed ? t.a : nullptr, stop, ka, nblocks, B.lds, err, sizeof err)) {
        if (timed) S.pool.push_back({t.a, t.b});
        return rc;
    }
    if (timed) S.pending.push_back(t);
    S.wait_ev = stop;
    n_launches++;
    S.stream_dirty = true;
    return 0;
}

// ---------------------------------------------------------------------------------- worker control (host)
inline void bar_fence() {
    std::atomic_thread_fence(std::memory_order_release);
#if defined(__x86_64__)
    __builtin_ia32_sfence();   // write-combining buffers drained: stores through the BAR leave in program order
#endif
}

int HipBackend::worker_start(int D, int alg) {
    Worker &W = worker;
    if (W.running && W.D == D && W.alg == alg) {
        // an idle worker leaves by itself after 10 s without a new item (every wave needs an exit the host cannot
        // withhold): after a pause of more than 1 s retire it and start a fresh one rather than trust a half-gone grid
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - W.last_push).count() < 1.0) return 0;
    }
    if (W.running) if (int rc = worker_stop()) return rc;
    if (!W.stream) {
        HIPCHK(hipStreamCreateWithFlags(&W.stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&W.ev_a));
        HIPCHK(hipEventCreate(&W.ev_b));
        if (W.qmem.alloc_fine(sizeof(WorkQ)) != hipSuccess) { (void)hipGetLastError(); W.disabled = true; return 1; }
        HIPCHK(W.ticket.alloc(64));
        const char *e = getenv("SPG_WORKER_WGS");
        if (e && atoi(e) > 0) W.wgs = atoi(e);
        if ((e = getenv("SPG_WORKER_BELLS")) && atoi(e) >= 1 && atoi(e) <= kBells) W.bells = atoi(e);
        if ((e = getenv("SPG_WORKER_LAZY")) && atoi(e) >= 0) W.lazy = atoi(e);
    }
    WorkQ *q = W.q();
    for (int c = 0; c < W.bells; c++) q->tail[c * kBellStride] = 0;     // through the BAR
    q->stop = 0;
    bar_fence();
    W.tail = 0; W.bytes = 0; W.blankets = 0;
    HIPCHK(hipMemsetAsync(W.ticket.p, 0, 64, W.stream));
    // LDS of the largest blanket a worker takes: n <= kWaveMax, one removed vertex, the two-wavefront carve-up
    Layout L = make_layout(D, 128, kWorkerMaxN / D, 1, alg, SPG_TOPO_TREE, 0);
    const size_t lds = (size_t)(L.small_doubles + L.mat_doubles) * 8;
    const long long idle_ticks = 10LL * 100000000LL;   // 10 s of the 100 MHz wall clock
    if (int rc = hip_worker_launch(D, W.wgs, lds, W.stream, W.ev_a, W.ev_b, q, (unsigned long long *)W.ticket.p, idle_ticks, W.bells, W.lazy, err, sizeof err)) return rc;
    W.running = true; W.D = D; W.alg = alg;
    W.last_push = std::chrono::steady_clock::now();
    n_launches++;
    return 0;
}

int HipBackend::worker_stop() {
    Worker &W = worker;
    if (!W.running) return 0;
    W.q()->stop = 1;
    bar_fence();
    HIPCHK(hipStreamSynchronize(W.stream));
    W.running = false;
    if (profiling) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, W.ev_a, W.ev_b) == hipSuccess) {
            prof_worker_ms += ms; prof_worker_bytes += W.bytes; prof_worker_runs++; prof_worker_blankets += W.blankets;
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------------- one round
// The batch goes to the persistent worker: packets (layout: blanket_worker, spg_kernels.hip) through the BAR, then the
// item slots, then the doorbells. 0 = the whole batch is with the worker, 1 = no worker on this system after all
// (fine-grained memory refused): launch it, < 0 error.
int HipBackend::push_to_worker(Slot &S, const spg_round_desc *rd, void *arena) {
    const spg_options &o = *rd->opts;
    const int D = o.pose_dim;
    const size_t n_push = (size_t)rd->count;
    bool fine = true;
    if (int rc = ensure_fine(S.pkt, n_push * (size_t)kPktWords * 8, (size_t)512 * kPktWords * 8, &fine)) return rc;
    if (!fine) worker.disabled = true;
    if (int rc = ensure_pinned(S.mail, (size_t)rd->mail_len * 8, true)) return rc;
    if (worker.disabled) return 1;
    if (int wrc = worker_start(D, SPG_ALG_NFR)) return wrc;
    Worker &W = worker;
    WorkQ *q = W.q();
    unsigned long long *pbase = (unsigned long long *)S.pkt.p;
    const double *hmail = (const double *)S.mail.h;
    S.final_word = SPG_FINAL_WORD(rd->tag);
    double wbytes = 0;
    for (size_t i = 0; i < n_push; i++) {
        const int32_t b = rd->first + (int32_t)i;
        const spg_blanket_desc &bd = rd->blankets[b];
        unsigned long long pkt[kPktWords];
        int nev = 0;
        const int words = worker_packet_words(bd, rd, &nev);
        auto pack = [](int lo, int hi) { return (unsigned long long)(uint32_t)lo | ((unsigned long long)(uint32_t)hi << 32); };
        pkt[0] = (unsigned long long)(uintptr_t)arena;
        pkt[1] = (unsigned long long)(uintptr_t)S.mail.d;
        pkt[2] = (unsigned long long)rd->mail_base;
        pkt[3] = (unsigned long long)bd.out_off; pkt[4] = (unsigned long long)bd.new_off; pkt[5] = (unsigned long long)bd.tinfo_off;
        pkt[6] = pack(bd.n_vert, bd.n_remove); pkt[7] = pack(bd.n_edge, bd.n_new_max); pkt[8] = pack(bd.n_new_vert_max, bd.pad_);
        pkt[9] = pack(o.topology, o.flags); pkt[10] = pack(o.lin_point, rd->tag);
        memcpy(&pkt[11], &o.chord_ratio, 8);
        pkt[12] = pack(words, nev | (worker_stamp ? 0x40000000 : 0));
        int w = kPktHdr;
        for (int v = 0; v < bd.n_vert; v++) pkt[w++] = (unsigned long long)rd->vert_pose_off[bd.vert_begin + v];
        int32_t *evp = (int32_t *)(pkt + kPktHdr + bd.n_vert + 3 * bd.n_edge);
        int evn = 0;
        for (int e = bd.edge_begin; e < bd.edge_begin + bd.n_edge; e++) {
            spg_edge_ref er = rd->edges[e];
            for (int t = 0; t < er.nv; t++) evp[evn + t] = rd->edge_vert[er.vbegin + t];
            er.vbegin = evn;
            evn += er.nv;
            memcpy(&pkt[w], &er, 24);
            w += 3;
        }
        if (evn & 1) evp[evn] = 0;
        wbytes += blanket_alg_bytes(D, bd, rd);
        unsigned long long *dst = pbase + i * (size_t)kPktWords;
        memcpy(dst, pkt, (size_t)words * 8);                       // through the BAR (write-combined)
        q->item[(W.tail + i) % kQCap] = (unsigned long long)(uintptr_t)dst;
        S.finals.push_back(hmail + (bd.out_off - rd->mail_base) + 5);
    }
    bar_fence();
    W.tail += n_push;
    for (int c = 0; c < W.bells; c++) q->tail[c * kBellStride] = W.tail;   // the doorbells
    bar_fence();
    W.last_push = std::chrono::steady_clock::now();
    W.bytes += wbytes; W.blankets += (long long)n_push;
    if (echo_test) {
        // diagnostic: doorbell -> ready word of the batch's first blanket, on the host clock
        const volatile double *rw = S.finals.front();
        const double want_r = SPG_READY_WORD(rd->tag), want_f = SPG_FINAL_WORD(rd->tag);
        auto t0 = std::chrono::steady_clock::now();
        while (*rw != want_r && *rw != want_f) { if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 1.0) break; }
        static double acc = 0; static long cnt = 0;
        acc += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); cnt++;
        if (cnt % 252 == 0) { fprintf(stderr, "worker echo test: doorbell -> first blanket ready %.1f us (avg over %ld batches of ~%zu)\n", acc / cnt, cnt, n_push); acc = 0; cnt = 0; }
    }
    return 0;
}

// ---- the round's descriptors and the launch lists (bins 0..4, then the generic list) where the kernels read them:
//  - small launch, large-BAR system: the host stores them straight into (fine-grained) device memory —
//    posted writes ahead of the doorbell, no copy engine hop, and the kernel reads local HBM;
//  - small launch otherwise: the kernel reads them from the mapped pinned staging buffer over PCIe;
//  - large launch: one host->device copy from the staging buffer.
int HipBackend::stage_descriptors(Slot &S, const spg_round_desc *rd, Staged &sd) {
    const size_t s_blk = sizeof(spg_blanket_desc) * (size_t)rd->n_blankets;
    const size_t s_vpo = sizeof(int64_t) * (size_t)rd->n_vert_total;
    const size_t s_er = sizeof(spg_edge_ref) * (size_t)rd->n_edge_total;
    const size_t s_ev = sizeof(int32_t) * (size_t)rd->n_edge_vert_total;
    const size_t s_list = sizeof(int32_t) * (size_t)rd->count;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    sd.o_blk = 0; sd.o_vpo = sd.o_blk + al(s_blk); sd.o_er = sd.o_vpo + al(s_vpo); sd.o_ev = sd.o_er + al(s_er); sd.o_list = sd.o_ev + al(s_ev);
    const size_t tot = sd.o_list + al(s_list);
    const bool small = (long long)rd->count <= (long long)mapped_limit;
    bool via_bar = small && large_bar && bar_ok;
    if (via_bar) {
        if (int rc = ensure_fine(S.bar, tot, (size_t)1 << 16, &via_bar)) return rc;
        if (!via_bar) large_bar = false;   // fall back to the mapped staging buffer
    }
    char *st;
    if (via_bar) {
        st = (char *)S.bar.p;   // write-only from the host
    } else {
        if (int rc = ensure_pinned(S.stage, tot, true, S.stream)) return rc;
        if (!small) if (int rc = ensure(S, S.desc, tot)) return rc;
        st = (char *)S.stage.h;
    }
    memcpy(st + sd.o_blk, rd->blankets, s_blk);
    memcpy(st + sd.o_vpo, rd->vert_pose_off, s_vpo);
    memcpy(st + sd.o_er, rd->edges, s_er);
    if (s_ev) memcpy(st + sd.o_ev, rd->edge_vert, s_ev);
    staged_list(S.plan, (int32_t *)(st + sd.o_list));
    if (via_bar) {
        bar_fence();   // write-combining buffers drained before the launch rings the doorbell
        sd.base = (char *)S.bar.p;
    } else if (small) {
        sd.base = (char *)S.stage.d;
    } else {
        sd.base = (char *)S.desc.p;
        HIPCHK(hipMemcpyAsync(S.desc.p, st, tot, hipMemcpyHostToDevice, S.stream));
    }
    return 0;
}

// ---- each non-empty bin, in order; `list` is the staged launch list (the bins' blankets back to back)
int HipBackend::launch_bins(Slot &S, KArgs &ka, const int32_t *list) {
    for (int i = 0; i < kPlanBins; i++) {
        const PlanBin &B = S.plan.bins[i];
        if (B.list.empty()) continue;
        ka.list = list;
        list += B.list.size();
        if (B.variant.gws) {
            if (int rc = ensure(S, S.gws, B.gws_stride * 8 * B.list.size())) return rc;
            ka.gws = (double *)S.gws.p;
            ka.gws_stride = (int64_t)B.gws_stride;
        }
        if (int rc = launch_bin(S, B, ka)) return rc;
    }
    return 0;
}

// The blanket as a small graph for the dense drivers (spg_dense.hip): local vertex = blanket-local index, pos_of(l) its
// scalar offset in the dense matrix (-1 = fixed), vpo[l] its pose offset; edges as staged for the kernels.
struct LocalGraph {
    std::vector<int32_t> pos, rowptr, inc;
    DenseGraphIn in;
    template <class PosOf>
    LocalGraph(int D, const spg_blanket_desc &bd, const spg_round_desc *rd, const void *arena, const int64_t *vpo, PosOf pos_of)
        : pos(bd.n_vert), rowptr(bd.n_vert + 1, 0) {
        for (int l = 0; l < bd.n_vert; l++) pos[l] = pos_of(l);
        std::vector<std::vector<int32_t>> per(bd.n_vert);
        for (int e = 0; e < bd.n_edge; e++) {
            const spg_edge_ref &er = rd->edges[bd.edge_begin + e];
            for (int t = 0; t < er.nv; t++) {
                const int32_t l = rd->edge_vert[er.vbegin + t];
                if (per[l].empty() || per[l].back() != e) per[l].push_back(e);
            }
        }
        for (int l = 0; l < bd.n_vert; l++) { inc.insert(inc.end(), per[l].begin(), per[l].end()); rowptr[l + 1] = (int32_t)inc.size(); }
        in.D = D; in.nv = bd.n_vert; in.ne = bd.n_edge;
        in.pos = pos.data(); in.vpo = vpo; in.rowptr = rowptr.data(); in.inc = inc.data();
        in.er = rd->edges + bd.edge_begin; in.ev = rd->edge_vert; in.n_ev = rd->n_edge_vert_total; in.dev_arena = arena;
    }
    LocalGraph(const LocalGraph &) = delete;
};

// ---- Local linearisation point for the blankets of the generic kernel (pre-pass, see local_point_kernel): scratch poses,
// closed-form re-initialisation on the device, else the reference's 10 LM iterations with the first removed vertex fixed —
// the dense LM of optimize() on the blanket as a small graph, host-driven, one blanket after the other — and a
// second table of pose offsets that points the generic kernel at the scratch blocks.
int HipBackend::local_prepass(Slot &S, const spg_round_desc *rd, void *arena, IpArgs &ia) {
    const std::vector<int32_t> &ip_list = S.plan.ip_list;
    const int D = rd->opts->pose_dim, PSl = (D == 6) ? 7 : 3;
    const size_t nl = ip_list.size();
    std::vector<int64_t> lp_off(nl);
    int64_t lp_tot = 0;
    for (size_t i = 0; i < nl; i++) { lp_off[i] = lp_tot; lp_tot += (int64_t)rd->blankets[ip_list[i]].n_vert * PSl; }
    const size_t meta_bytes = nl * 8 + nl * 4 + (size_t)rd->n_vert_total * 8 + 64;
    if (int rc = ensure(S, S.lpose, (size_t)lp_tot * 8 + 64)) return rc;
    if (int rc = ensure(S, S.lmeta, meta_bytes)) return rc;
    int64_t *d_lp_off = (int64_t *)S.lmeta.p, *d_vpo2 = d_lp_off + nl;
    int32_t *d_flag = (int32_t *)(d_vpo2 + rd->n_vert_total);
    const int64_t scratch0 = ((intptr_t)S.lpose.p - (intptr_t)arena) / 8;   // the scratch block as an "arena offset"
    std::vector<int64_t> vpo2(rd->vert_pose_off, rd->vert_pose_off + rd->n_vert_total);
    for (size_t i = 0; i < nl; i++) {
        const spg_blanket_desc &bd = rd->blankets[ip_list[i]];
        for (int v = 0; v < bd.n_vert; v++) vpo2[(size_t)bd.vert_begin + v] = scratch0 + lp_off[i] + (int64_t)v * PSl;
    }
    HIPCHK(hipMemcpyAsync(d_lp_off, lp_off.data(), nl * 8, hipMemcpyHostToDevice, S.stream));
    HIPCHK(hipMemcpyAsync(d_vpo2, vpo2.data(), (size_t)rd->n_vert_total * 8, hipMemcpyHostToDevice, S.stream));
    if (int rc = hip_local_point_launch(D, S.stream, (int)nl, (const double *)arena, (double *)S.lpose.p, ia.blk, ia.vpo, ia.er, ia.ev, ia.list,
                                        (const int64_t *)d_lp_off, d_flag, err, sizeof err)) return rc;
    std::vector<int32_t> h_flag(nl);
    HIPCHK(hipMemcpyAsync(h_flag.data(), d_flag, nl * 4, hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    for (size_t i = 0; i < nl; i++) {
        if (h_flag[i]) continue;
        const spg_blanket_desc &bd = rd->blankets[ip_list[i]];
        // vertex 0 fixed, the poses in the scratch block
        std::vector<int64_t> lvpo(bd.n_vert);
        for (int l = 0; l < bd.n_vert; l++) lvpo[l] = scratch0 + lp_off[i] + (int64_t)l * PSl;
        LocalGraph g(D, bd, rd, arena, lvpo.data(), [&](int l) { return l == 0 ? -1 : (l - 1) * D; });
        spg_optimize_stats lm_stats{};
        if (int lrc = hip_dense_optimize((void *)S.stream, g.in, D * (bd.n_vert - 1), 10, lm_stats, err, sizeof err)) return lrc;
    }
    ia.vpo = (const int64_t *)d_vpo2;
    ia.lin_point = SPG_LIN_GLOBAL;   // the scratch poses ARE the local linearisation point: taken as they are
    return 0;
}

// ---- the blankets of the generic kernel (interior point / closed form, spg_nfr_ip.hip); `list` is their launch list
int HipBackend::launch_generic(Slot &S, const spg_round_desc *rd, void *arena, const KArgs &ka, const int32_t *list) {
    const RoundPlan &P = S.plan;
    if (P.ip_list.empty()) return 0;
    const spg_options &o = *rd->opts;
    const size_t ws_bytes = (size_t)P.ip_stride * 8 * P.ip_list.size();
    if (int rc = ensure(S, S.ipws, ws_bytes)) return rc;
    // The workspace is reused from launch to launch and from graph to graph: cleared, so that what a blanket finds in its
    // slice never depends on what ran before it in the process (a run of several graphs through one context died with a
    // core dump in round 2 where each graph on its own passes; hipMalloc'ed memory is not zeroed either).
    HIPCHK(hipMemsetAsync(S.ipws.p, 0, ws_bytes, S.stream));
    IpArgs ia{};
    ia.arena = (double *)arena; ia.blk = ka.blk; ia.vpo = ka.vpo; ia.er = ka.er; ia.ev = ka.ev;
    ia.list = list;
    ia.ws = (double *)S.ipws.p; ia.ws_stride = P.ip_stride; ia.mail = ka.mail; ia.mail_base = rd->mail_base;
    ia.topology = o.topology; ia.lin_point = o.lin_point; ia.tag = rd->tag; ia.chord_ratio = o.chord_ratio;
    ia.factor_descent = (o.flags & SPG_FLAG_NFR_FACTOR_DESCENT) ? 1 : 0; ia.fd_rel_tol = fd_rel_tol; ia.fd_max_cycles = fd_max_cycles;
    if (o.lin_point != SPG_LIN_GLOBAL) if (int rc = local_prepass(S, rd, arena, ia)) return rc;
    if (int rc = hip_nfr_ip_launch((void *)S.stream, o.pose_dim, ia, (int)P.ip_list.size(), P.ip_closed, P.ip_hot)) { snprintf(err, sizeof err, "launch of the interior-point kernel failed"); return rc; }
    // (this kernel comes AFTER the event a bin launch left in wait_ev: waiting for the slot must mean the whole stream.
    //  Until round 3 wait_slot returned when the bin kernel was done — with a cluster of 150 vertices still running in
    //  this one, the commit read whatever the mailbox held at its record's place: silently wrong graphs on parking.g2o
    //  under CliqueyDense, and a segmentation fault when the stale words were not zeros.)
    S.wait_ev = nullptr;
    S.stream_dirty = true;
    S.busy = true;
    return 0;
}

// ---- large GLC Dense blankets: dense in HBM, O(n^3) parts on the fp64 matrix cores, one at a time
int HipBackend::run_big_blankets(Slot &S, const spg_round_desc *rd, void *arena, double *mail_dev) {
    const int D = rd->opts->pose_dim;
    for (int32_t b : S.plan.big_list) {
        const spg_blanket_desc &bd = rd->blankets[b];
        const int k = bd.n_vert - bd.n_remove, m = bd.n_remove;
        // vertices = blanket-local indices (removed first, padded to the 64-wide tiles of the pipeline)
        const int nm = D * m, Nm = (nm + 63) / 64 * 64;
        LocalGraph g(D, bd, rd, arena, rd->vert_pose_off + bd.vert_begin, [&](int l) { return l < m ? l * D : Nm + (l - m) * D; });
        double *orec = mail_dev ? (mail_dev + (bd.out_off - rd->mail_base)) : ((double *)arena + bd.out_off);
        double secs = 0, flops = 0;
        // (no per-blanket KLD on this path: under SPG_FLAG_GLC_KLD the blanket says so in its info word)
        const int info_bits = (rd->opts->flags & SPG_FLAG_GLC_KLD) ? SPG_INFO_GLC_KLD_SKIPPED : 0;
        if (int brc = hip_big_glc_dense((void *)S.stream, g.in, m, k, Nm, bd.new_off, orec, bd.n_new_max, rd->tag, info_bits, &secs, &flops, err, sizeof err)) return brc;
        prof_big_ms += 1e3 * secs; prof_big_flops += flops; prof_big_count++;
        prof_big_nmax = std::max(prof_big_nmax, D * (k + m));
        S.wait_ev = nullptr;   // (as above: the slot is done when the stream is)
        S.stream_dirty = true;
    }
    return 0;
}

int HipBackend::run_round(void *arena, const spg_round_desc *rd) {
    if (rd->count <= 0) return 0;
    Slot &S = slots[rd->slot & (NSLOT - 1)];
    const spg_options &o = *rd->opts;
    if (o.pose_dim != 3 && o.pose_dim != 6) return SPG_EINVAL;
    if (int rc = make_current()) return rc;
    // the previous launch of this slot must have drained before its staging buffer is rewritten
    // (already the case when the host has just harvested the slot's late results)
    if (S.busy) if (int rc = wait_slot(S)) return rc;
    drain_profile(S);
    S.busy = true;
    // (the worker decision comes first: a batch that goes to the worker needs neither bins nor launch descriptors)
    PlanConfig cfg;
    cfg.lds_limit = lds_limit; cfg.force_one_wave = force_one_wave; cfg.large_bar = large_bar;
    cfg.worker_enabled = worker_env && !worker.disabled; cfg.force_big = force_big; cfg.profiling = profiling;
    const WorkerState ws{++batches_in_call, worker_cooldown, worker.running};
    plan_worker(rd, cfg, ws, S.plan);
    worker_cooldown = S.plan.cooldown;
    if (S.plan.to_worker) {
        const int rc = push_to_worker(S, rd, arena);
        if (rc <= 0) return rc;
    }
    if (int rc = worker_stop()) return rc;                           // a launch follows: the worker must not be in its way
    if (int rc = plan_launch(rd, cfg, S.plan, err, sizeof err)) return rc;
    Staged sd{};
    if (int rc = stage_descriptors(S, rd, sd)) return rc;
    double *mail_dev = nullptr;
    if (rd->mail_len > 0) {
        if (int rc = ensure_pinned(S.mail, (size_t)rd->mail_len * 8, true)) return rc;
        mail_dev = (double *)S.mail.d;
    }
    KArgs ka;
    ka.arena = (double *)arena;
    ka.blk = (const spg_blanket_desc *)(sd.base + sd.o_blk);
    ka.vpo = (const int64_t *)(sd.base + sd.o_vpo);
    ka.er = (const spg_edge_ref *)(sd.base + sd.o_er);
    ka.ev = (const int32_t *)(sd.base + sd.o_ev);
    ka.list = nullptr;
    ka.mail = mail_dev;
    ka.mail_base = rd->mail_base;
    ka.gws = nullptr; ka.gws_stride = 0;
    ka.topology = o.topology; ka.algorithm = o.algorithm; ka.flags = o.flags; ka.chord_ratio = o.chord_ratio; ka.lin_point = o.lin_point; ka.tag = rd->tag;
    const int32_t *list = (const int32_t *)(sd.base + sd.o_list);
    size_t n_binned = 0;
    for (const PlanBin &B : S.plan.bins) n_binned += B.list.size();
    if (int rc = launch_bins(S, ka, list)) return rc;
    if (int rc = launch_generic(S, rd, arena, ka, list + n_binned)) return rc;
    return run_big_blankets(S, rd, arena, mail_dev);
}

// ---------------------------------------------------------------------------------- the spg_backend callbacks
int hip_run_round(void *user, void *arena, const spg_round_desc *rd) { return ((HipBackend *)user)->run_round(arena, rd); }

void *hip_alloc(void *user, int64_t doubles) {
    HipBackend *hb = (HipBackend *)user;
    void *p = nullptr;
    if (hipSetDevice(hb->device) != hipSuccess) return nullptr;
    if (hipMalloc(&p, (size_t)doubles * 8) != hipSuccess) return nullptr;
    return p;
}
void hip_release(void *user, void *p) {
    HipBackend *hb = (HipBackend *)user;
    (void)hb->worker_stop();   // hipFree waits for the whole device
    (void)hipStreamSynchronize(hb->slots[0].stream);
    (void)hipFree(p);
}
int hip_upload(void *user, void *dst, const double *src, int64_t doubles) {
    HipBackend *hb = (HipBackend *)user;
    char *err = hb->err;
    if (int rcw = hb->worker_stop()) return rcw;
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)doubles * 8, hipMemcpyHostToDevice, hb->slots[0].stream));
    HIPCHK(hipStreamSynchronize(hb->slots[0].stream));
    return 0;
}
int hip_download(void *user, double *dst, const void *src, int64_t doubles) {
    HipBackend *hb = (HipBackend *)user;
    char *err = hb->err;
    if (int rcw = hb->worker_stop()) return rcw;
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)doubles * 8, hipMemcpyDeviceToHost, hb->slots[0].stream));
    HIPCHK(hipStreamSynchronize(hb->slots[0].stream));
    return 0;
}
int hip_sync(void *user) {
    HipBackend *hb = (HipBackend *)user;
    char *err = hb->err;
    for (auto &S : hb->slots) {
        if (S.busy || S.wait_ev || !S.finals.empty()) { if (int rcw = hb->wait_slot(S)) return rcw; }
        else HIPCHK(hipStreamSynchronize(S.stream));   // copies issued outside hip_run_round
        hb->drain_profile(S);
    }
    // a full synchronisation leaves the device idle: the persistent worker retires (it restarts on demand)
    hb->batches_in_call = 0;
    return hb->worker_stop();
}
int hip_sync_slot(void *user, int slot) {
    HipBackend *hb = (HipBackend *)user;
    HipBackend::Slot &S = hb->slots[slot & (HipBackend::NSLOT - 1)];
    if (int rcw = hb->wait_slot(S)) return rcw;
    hb->drain_profile(S);
    return 0;
}

const double *hip_mailbox(void *user) { return (const double *)((HipBackend *)user)->slots[0].mail.h; }
const double *hip_mailbox_slot(void *user, int slot) { return (const double *)((HipBackend *)user)->slots[slot & (HipBackend::NSLOT - 1)].mail.h; }

}  // namespace

int hip_backend_create(int device, spg_backend *out, char *errbuf, size_t errlen) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        snprintf(errbuf, errlen, "no HIP device available (count=%d, requested=%d): %s — libspg_hip has no CPU fallback",
                 ndev, device, e == hipSuccess ? "ok" : hipGetErrorString(e));
        return SPG_ENODEV;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { snprintf(errbuf, errlen, "hipGetDeviceProperties failed"); return SPG_ENODEV; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        snprintf(errbuf, errlen, "device %d is %s; this library carries gfx950 (MI355X) code objects only", device, prop.gcnArchName);
        return SPG_ENODEV;
    }
    HipBackend *hb = new HipBackend;
    hb->device = device;
    bool okc = hipSetDevice(device) == hipSuccess;
    for (auto &S : hb->slots) okc = okc && hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking) == hipSuccess &&
                                          hipEventCreateWithFlags(&S.done, hipEventDisableTiming) == hipSuccess;
    if (!okc) {
        snprintf(errbuf, errlen, "cannot create HIP stream on device %d", device);
        delete hb;
        return SPG_EHIP;
    }
    hb->lds_limit = (int)prop.sharedMemPerBlock > 0 ? (int)std::min<size_t>(prop.sharedMemPerBlock, 160 * 1024) : 64 * 1024;
    {
        int lb = 0;
        hb->large_bar = hipDeviceGetAttribute(&lb, hipDeviceAttributeIsLargeBar, device) == hipSuccess && lb != 0;
    }
    out->user = hb;
    out->alloc = hip_alloc;
    out->release = hip_release;
    out->upload = hip_upload;
    out->download = hip_download;
    out->run_round = hip_run_round;
    out->synchronize = hip_sync;
    out->mailbox = hip_mailbox;
    out->synchronize_slot = hip_sync_slot;
    out->mailbox_slot = hip_mailbox_slot;
    return 0;
}

// (the buffers release themselves with the backend, after the streams they were used on are idle and gone)
void hip_backend_destroy(spg_backend *b) {
    HipBackend *hb = (HipBackend *)b->user;
    if (!hb) return;
    (void)hipSetDevice(hb->device);
    (void)hb->worker_stop();
    for (auto &S : hb->slots) (void)hipStreamSynchronize(S.stream);
    hip_big_release_scratch();
    if (hb->worker.ev_a) (void)hipEventDestroy(hb->worker.ev_a);
    if (hb->worker.ev_b) (void)hipEventDestroy(hb->worker.ev_b);
    if (hb->worker.stream) (void)hipStreamDestroy(hb->worker.stream);
    for (auto &S : hb->slots) {
        if (S.done) (void)hipEventDestroy(S.done);
        for (auto &t : S.pending) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
        for (auto &pr : S.pool) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        (void)hipStreamDestroy(S.stream);
    }
    delete hb;
    b->user = nullptr;
}

void *hip_backend_stream(spg_backend *b) { return b->user ? (void *)((HipBackend *)b->user)->slots[0].stream : nullptr; }
const char *hip_backend_error(spg_backend *b) { return b->user ? ((HipBackend *)b->user)->err : ""; }
int hip_backend_device(spg_backend *b) { return b->user ? ((HipBackend *)b->user)->device : -1; }
int hip_backend_launches(spg_backend *b) { return b->user ? ((HipBackend *)b->user)->n_launches.load() : 0; }
void hip_backend_profile(spg_backend *b, int enable) {
    HipBackend *hb = (HipBackend *)b->user;
    if (!hb) return;
    hb->profiling = enable != 0;
    hb->prof_stride = enable > 1 ? enable : 1;   // enable = n > 1: HIP events around every n-th launch only
    hb->prof_tick = 0;
    for (auto &S : hb->slots) { S.prof_ms = S.prof_bytes = 0; S.prof_launches = S.prof_blankets = 0; }
    hb->prof_worker_ms = hb->prof_worker_bytes = 0; hb->prof_worker_runs = hb->prof_worker_blankets = 0;
    hb->prof_big_ms = hb->prof_big_flops = 0; hb->prof_big_count = 0; hb->prof_big_nmax = 0;
}
void hip_backend_profile_read(spg_backend *b, double *ms, double *bytes, long long *launches, long long *blankets) {
    HipBackend *hb = (HipBackend *)b->user;
    if (!hb) return;
    *ms = *bytes = 0; *launches = *blankets = 0;
    for (auto &S : hb->slots) { *ms += S.prof_ms; *bytes += S.prof_bytes; *launches += S.prof_launches; *blankets += S.prof_blankets; }
}
void hip_backend_profile_read_worker(spg_backend *b, double *ms, double *bytes, long long *runs, long long *blankets) {
    HipBackend *hb = (HipBackend *)b->user;
    if (!hb) return;
    *ms = hb->prof_worker_ms; *bytes = hb->prof_worker_bytes; *runs = hb->prof_worker_runs; *blankets = hb->prof_worker_blankets;
}
void hip_backend_profile_read_big(spg_backend *b, double *ms, double *flops, long long *count, int *nmax) {
    HipBackend *hb = (HipBackend *)b->user;
    if (!hb) return;
    *ms = hb->prof_big_ms; *flops = hb->prof_big_flops; *count = hb->prof_big_count; *nmax = hb->prof_big_nmax;
}
void hip_backend_set_factor_descent(spg_backend *b, double rel_tol, int max_cycles) {
    if (!b->user) return;
    HipBackend *hb = (HipBackend *)b->user;
    hb->fd_rel_tol = rel_tol; hb->fd_max_cycles = max_cycles;
}
int hip_backend_end_of_call(spg_backend *b) {
    HipBackend *hb = (HipBackend *)b->user;
    if (!hb) return 0;
    hb->batches_in_call = 0;
    return hb->worker_stop();
}

int hip_stream_open(spg_backend *b, int D, int slots, int mail_stride, StreamPort *out) {
    HipBackend *hb = (HipBackend *)b->user;
    if (!hb || !out || slots < 1 || slots > kQCap / 2 || (D != 3 && D != 6)) return SPG_EINVAL;
    if (!hb->worker_env || !hb->large_bar || hb->worker.disabled || hb->force_one_wave) return 1;
    if (int rc = hb->make_current()) return rc;
    // nothing of an earlier batch may still be running on the launch slots (their kernels would queue behind the worker)
    for (auto &S : hb->slots) if (S.busy || S.wait_ev || !S.finals.empty()) { if (int rcw = hb->wait_slot(S)) return rcw; hb->drain_profile(S); }
    bool fine = true;
    if (int rc = hb->ensure_fine(hb->st_pkt, (size_t)slots * kPktWords * 8, 0, &fine)) return rc;
    if (!fine) return 1;
    if (int rc = hb->ensure_pinned(hb->st_mail, (size_t)slots * (size_t)mail_stride * 8, false)) return rc;
    int wrc = hb->worker_start(D, SPG_ALG_NFR);
    if (wrc) return wrc;
    if (hb->worker.disabled) return 1;
    hb->batches_in_call += 3;   // (batches that follow in this call may go to the running worker right away)
    out->pkt = (unsigned long long *)hb->st_pkt.p;
    out->q = hb->worker.q();
    out->tail = hb->worker.tail;
    out->bells = hb->worker.bells;
    out->h_mail = (const double *)hb->st_mail.h;
    out->d_mail = (unsigned long long)(uintptr_t)hb->st_mail.d;
    out->mail_stride = mail_stride;
    out->slots = slots;
    return 0;
}

void hip_stream_close(spg_backend *b, const StreamPort *port, double alg_bytes, long long blankets) {
    HipBackend *hb = (HipBackend *)b->user;
    if (!hb || !port) return;
    hb->worker.tail = port->tail;
    hb->worker.bytes += alg_bytes;
    hb->worker.blankets += blankets;
    hb->worker.last_push = std::chrono::steady_clock::now();
}

}  // namespace spg
