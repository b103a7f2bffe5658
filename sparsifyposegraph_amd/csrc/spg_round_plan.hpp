// csrc/spg_round_plan.hpp — where every blanket of one round goes: to the persistent worker, to one of the five LDS bins
// of blanket_kernel (and which kernel variant serves the bin), to the generic interior-point / closed-form kernel
// (spg_nfr_ip.hip), to the large-blanket dense pipeline (spg_dense.hip), or nowhere (SPG_ECAPACITY).
//
// Pure arithmetic on the round descriptor, the options and a few backend flags: no HIP call, no allocation beyond the
// growth of the caller's lists, so the rules can be exercised without a device (tests/cpp/plan_demo.cpp). The backend
// (spg_hip_backend.cpp) runs plan_worker, hands the batch over or retires the worker, then runs plan_launch.
#pragma once
#include <algorithm>
#include <cstdio>
#include <vector>
#include "spg_blanket_layout.hpp"
#include "spg_internal.h"

#pragma GCC visibility push(hidden)
namespace spg {

struct PlanConfig {
    int lds_limit = 160 * 1024;     // dynamic LDS one workgroup may ask for
    bool force_one_wave = false;    // SPG_ONE_WAVE=1
    bool large_bar = false;         // the host can store straight into device memory
    bool worker_enabled = true;     // SPG_WORKER != 0 and the worker's queue could be allocated
    bool force_big = false;         // SPG_FORCE_BIG=1
    bool profiling = false;         // account the algorithmic bytes of every bin
};
struct WorkerState {
    int batches_in_call = 0;        // batches since the last full synchronisation, this one included
    int cooldown = 0;               // batches to go before the worker is considered again
    bool running = false;
};

constexpr int kPlanBins = 5;
struct PlanBin {
    std::vector<int32_t> list;      // blanket indices, in round order
    int kmax = 0, mmax = 0, smax = 0;
    double bytes = 0;               // algorithmic bytes (profiling only)
    // what launches the bin (non-empty bins only): bins 0..3 keep their tiles in LDS, the last one in a global workspace
    // of gws_stride doubles per blanket
    BlanketVariant variant{};
    size_t lds = 0, gws_stride = 0;
};
// (kept per launch slot by the backend: the lists keep their capacity, so a round allocates nothing)
struct RoundPlan {
    bool to_worker = false;
    int cooldown = 0;               // the backend's cool-down after this round
    PlanBin bins[kPlanBins];
    std::vector<int32_t> ip_list;   // generic kernel: interior point, correlated patterns, clusters under Local, k beyond LDS
    int ip_closed = 0;              // ... of which have a closed form
    int64_t ip_stride = 0, ip_hot = 0;
    std::vector<int32_t> big_list;  // GLC Dense blankets for the dense HBM pipeline
};

// algorithmic HBM bytes of one blanket: poses + (2 x i32 + record) per edge + new records + (kld f64 + status i32)
inline double blanket_alg_bytes(int D, const spg_blanket_desc &bd, const spg_round_desc *rd) {
    double by = 8.0 * ((D == 6) ? 7 : 3) * bd.n_vert + 12.0;
    for (int e = bd.edge_begin; e < bd.edge_begin + bd.n_edge; e++) by += 4.0 * rd->edges[e].nv + 8.0 * rd->edges[e].len;
    return by + 8.0 * bd.new_len;
}

// words of the worker packet of one blanket (layout: blanket_worker, spg_kernels.hip)
inline int worker_packet_words(const spg_blanket_desc &bd, const spg_round_desc *rd, int *n_edge_vert = nullptr) {
    int nev = 0;
    for (int e = bd.edge_begin; e < bd.edge_begin + bd.n_edge; e++) nev += rd->edges[e].nv;
    if (n_edge_vert) *n_edge_vert = nev;
    return kPktHdr + bd.n_vert + 3 * bd.n_edge + (nev + 1) / 2;
}

// ---- narrow batch: hand the blankets to the persistent worker instead of launching
// While the worker runs nothing else is submitted to the device: HIP multiplexes streams onto a few hardware queues
// and a dispatch queued behind the never-ending worker kernel would wait for it. So a batch goes to the worker
// whole (every blanket eligible) or the worker is retired first and the batch is launched as before.
inline void plan_worker(const spg_round_desc *rd, const PlanConfig &cfg, const WorkerState &ws, RoundPlan &P) {
    const spg_options &o = *rd->opts;
    const int D = o.pose_dim;
    // (not for the first two batches after a synchronisation: a call that removes a handful of vertices, e.g. online
    //  decimation, is cheaper as a plain launch than as worker start + stop)
    bool to_worker = cfg.worker_enabled && cfg.large_bar && rd->mail_len > 0 && o.algorithm == SPG_ALG_NFR && o.topology == SPG_TOPO_TREE &&
                     o.lin_point == SPG_LIN_GLOBAL && (o.flags & ~SPG_FLAG_NFR_FACTOR_DESCENT) == 0 && rd->count <= 512 && !cfg.force_one_wave &&
                     ws.cooldown == 0 && (ws.batches_in_call > 2 || ws.running);
    P.cooldown = ws.cooldown > 0 ? ws.cooldown - 1 : 0;
    if (to_worker) {
        // eligible: pose-pose edges only, one removed vertex, n <= kWorkerMaxN, packet fits the staging area
        for (int b = rd->first; b < rd->first + rd->count && to_worker; b++) {
            const spg_blanket_desc &bd = rd->blankets[b];
            const int k = bd.n_vert - bd.n_remove;
            bool bin = true;
            for (int e = bd.edge_begin; e < bd.edge_begin + bd.n_edge; e++) bin &= (rd->edges[e].kind == SPG_EDGE_BINARY);
            to_worker = bin && bd.n_remove == 1 && k >= 1 && D * k <= kWorkerMaxN && worker_packet_words(bd, rd) <= kPktWords && bd.tinfo_off < 0;
        }
        if (!to_worker) P.cooldown = 8;   // mixed batches: stay with launches for a while rather than stop / start per batch
    }
    P.to_worker = to_worker;
}

// ---- bin the round's blankets by the LDS their tiles need
inline void plan_bins(const spg_round_desc *rd, const PlanConfig &cfg, RoundPlan &P) {
    const spg_options &o = *rd->opts;
    const int D = o.pose_dim;
    const size_t lim[kPlanBins - 1] = {24 * 1024, 40 * 1024, 80 * 1024, (size_t)cfg.lds_limit};
    for (int b = rd->first; b < rd->first + rd->count; b++) {
        const spg_blanket_desc &bd = rd->blankets[b];
        int k = bd.n_vert - bd.n_remove, m = bd.n_remove;
        // (binned with the carve-up of the widest team any LDS variant uses, so that no variant outgrows its bin)
        Layout L = make_layout(D, 256, k, m, o.algorithm, o.topology, bd.pad_);
        size_t need = (size_t)(L.small_doubles + L.mat_doubles) * 8;
        int bi = kPlanBins - 1;
        for (int i = 0; i < kPlanBins - 1; i++) if (need <= lim[i]) { bi = i; break; }
        PlanBin &B = P.bins[bi];
        B.list.push_back(b);
        if (cfg.profiling) B.bytes += blanket_alg_bytes(D, bd, rd);
        B.kmax = std::max(B.kmax, k);
        B.mmax = std::max(B.mmax, m);
        B.smax = std::max(B.smax, (int)bd.pad_);
    }
}

// Keeps in bin B the blankets for which stays(b) holds (stays() disposes of the others itself); the envelope of the bin
// is recomputed if one left.
template <class F>
void filter_bin(const spg_round_desc *rd, PlanBin &B, F &&stays) {
    size_t keep = 0;
    int kmax = 0, mmax = 0, smax = 0;
    for (int32_t b : B.list) {
        if (!stays(b)) continue;
        const spg_blanket_desc &bd = rd->blankets[b];
        B.list[keep++] = b;
        kmax = std::max(kmax, bd.n_vert - bd.n_remove); mmax = std::max(mmax, (int)bd.n_remove); smax = std::max(smax, (int)bd.pad_);
    }
    if (keep != B.list.size()) { B.list.resize(keep); B.kmax = kmax; B.mmax = mmax; B.smax = smax; }
}

// NFR blankets whose pattern (Dense / Subgraph with more than k-1 edges) has no closed form: interior point, its own
// kernel (spg_nfr_ip.hip), one workgroup per blanket after the bin launches. The same kernel's closed form takes the
// correlated patterns, any blanket that holds a correlated edge, clusters under the Local linearisation point (the
// blanket kernel's own Local branch is for one removed vertex) and blankets whose Chow-Liu pair tables and side buffers
// outgrow LDS even with the tiles in the L2 workspace (k beyond ~130; the generic kernel keeps everything in its
// workspace, k <= 256).
inline int plan_generic(const spg_round_desc *rd, const PlanConfig &cfg, RoundPlan &P, char *err, size_t errlen) {
    const spg_options &o = *rd->opts;
    const int D = o.pose_dim;
    if (o.algorithm != SPG_ALG_NFR) return 0;
    const bool cliquey = o.topology == SPG_TOPO_CLIQUEY_SUBGRAPH || o.topology == SPG_TOPO_CLIQUEY_DENSE;
    // SPG_FLAG_NFR_FACTOR_DESCENT: the blankets of the interior point go through factor descent (spg_nfr_fd.inc) — no Newton
    // system, so no kIpMaxVars, and a workspace without the (d^2 E)^2 Hessian
    const bool fd = (o.flags & SPG_FLAG_NFR_FACTOR_DESCENT) != 0;
    int rc = 0;
    for (int i = 0; i < kPlanBins && !rc; i++) {
        filter_bin(rd, P.bins[i], [&](int32_t b) {
            if (rc) return true;
            const spg_blanket_desc &bd = rd->blankets[b];
            const int k = bd.n_vert - bd.n_remove, m = bd.n_remove;
            const int E = nfr_ip_pattern_size(o.topology, o.chord_ratio, k);
            bool has_multi = false;
            for (int e = bd.edge_begin; e < bd.edge_begin + bd.n_edge; e++) has_multi |= rd->edges[e].kind == SPG_EDGE_MULTI;
            const bool ip = k >= 3 && !cliquey && E > k - 1;           // uncorrelated pattern without a closed form
            const bool local_cluster = o.lin_point != SPG_LIN_GLOBAL && m > 1 && k >= 2;
            bool too_big = false;
            if (i == kPlanBins - 1 && k >= 2) {
                const bool lm_ = o.lin_point != SPG_LIN_GLOBAL;
                Layout Lw = make_layout(D, lm_ ? 256 : 1024, k, m, o.algorithm, o.topology, bd.pad_);
                too_big = (size_t)Lw.small_doubles * 8 > (size_t)cfg.lds_limit;
            }
            if (!(ip || (cliquey && k >= 3) || (has_multi && k >= 2) || local_cluster || too_big)) return true;
            const int msub = (int)((1 + o.chord_ratio) * (k - 1));
            const bool masks = o.topology == SPG_TOPO_CLIQUEY_SUBGRAPH && msub < k * (k - 1) / 2;   // fillCliques on 64-bit vertex masks
            // (interior point: Newton systems up to 2 048 variables in LDS-resident forms, up to kIpMaxVars through the
            //  blocked factorisation — one workgroup, 0.1 s per Newton step at 2 400 variables, 1 s at 4 900, 5 s at 8 300)
            if ((ip && !fd && (int64_t)D * D * E > kIpMaxVars) || (masks && k > 64) || k > 256) {
                snprintf(err, errlen, "interior-point / correlated NFR: a blanket with k=%d kept vertices and %d new measurements is beyond the generic kernel (Newton systems up to %d variables; k <= 64 for CliqueySubgraph, 256 otherwise)", k, E, kIpMaxVars);
                rc = SPG_ECAPACITY;
                return true;
            }
            P.ip_list.push_back(b);
            if (!ip) P.ip_closed++;        // (closed form: every correlated pattern, trees with correlated input edges)
            int64_t hot = 0;
            P.ip_stride = std::max(P.ip_stride, (ip && fd) ? nfr_fd_workspace(D, k, m, E, &hot) : nfr_ip_workspace(D, k, m, E, ip ? 0 : 1, &hot));
            P.ip_hot = std::max(P.ip_hot, hot);
            return false;
        });
    }
    return rc;
}

// Blankets whose side buffers (Chow-Liu pair tables, GLC batch buffers) exceed LDS even with the tiles in the L2
// workspace: GLC Dense ones go through the dense HBM pipeline on the matrix cores (spg_dense.hip) after the bin
// launches, one at a time; for the others there is no path (SPG_ECAPACITY).
inline int plan_big(const spg_round_desc *rd, const PlanConfig &cfg, RoundPlan &P, char *err, size_t errlen) {
    const spg_options &o = *rd->opts;
    const int D = o.pose_dim;
    const bool has_big_path = o.algorithm == SPG_ALG_GLC && o.topology == SPG_TOPO_DENSE && o.lin_point == SPG_LIN_GLOBAL;
    if (cfg.force_big && has_big_path) {
        // every blanket with at least two kept vertices takes the dense pipeline (parity of that path on small blankets)
        for (PlanBin &B : P.bins) {
            size_t keep = 0;
            for (int32_t b : B.list) {
                if (rd->blankets[b].n_vert - rd->blankets[b].n_remove >= 2 && rd->blankets[b].n_edge > 0) P.big_list.push_back(b);
                else B.list[keep++] = b;
            }
            B.list.resize(keep);
        }
        std::sort(P.big_list.begin(), P.big_list.end());
        return 0;
    }
    int rc = 0;
    filter_bin(rd, P.bins[kPlanBins - 1], [&](int32_t b) {
        if (rc) return true;
        const spg_blanket_desc &bd = rd->blankets[b];
        const int k = bd.n_vert - bd.n_remove, m = bd.n_remove;
        Layout Lb = make_layout(D, 256, k, m, o.algorithm, o.topology, bd.pad_);
        if ((size_t)Lb.small_doubles * 8 <= (size_t)cfg.lds_limit) return true;
        if (!has_big_path) {
            snprintf(err, errlen, "blanket too large for LDS side buffers: k=%d m=%d (only GLC Dense blankets have a large-blanket path)", k, m);
            rc = SPG_ECAPACITY;
            return true;
        }
        P.big_list.push_back(b);
        return false;
    });
    return rc;
}

// ---- the kernel variant and the LDS of each non-empty bin
inline int plan_variants(const spg_round_desc *rd, const PlanConfig &cfg, RoundPlan &P, char *err, size_t errlen) {
    const spg_options &o = *rd->opts;
    const int D = o.pose_dim;
    const bool nfr = o.algorithm == SPG_ALG_NFR;
    // Local linearisation point: the kernel variant that carries the blanket-level LM
    const bool lm = nfr && (o.lin_point != SPG_LIN_GLOBAL);
    const int alg = o.algorithm == SPG_ALG_GLC ? SPG_ALG_GLC : lm ? SPG_ALG_NFR_LM : SPG_ALG_NFR;
    for (int i = 0; i < kPlanBins; i++) {
        PlanBin &B = P.bins[i];
        const size_t nb = B.list.size();
        if (nb == 0) continue;
        auto layout = [&](int nt) { return make_layout(D, nt, B.kmax, B.mmax, o.algorithm, o.topology, B.smax); };
        if (i == kPlanBins - 1) {
            // NFR: eight wavefronts per blanket — the tiles sit in L2, every step of the cooperative routines is a round of
            // ~1 us accesses, and only lanes hide that (parking.g2o: 3.1 -> ms per launch of such blankets)
            const bool wide = nfr && !lm && !cfg.force_one_wave;
            const Layout L = layout(wide ? 1024 : 256);
            B.variant = {D, wide ? 1024 : 256, true, alg};
            B.lds = (size_t)L.small_doubles * 8;
            if (B.lds > (size_t)cfg.lds_limit) { snprintf(err, errlen, "blanket too large for LDS side buffers: k=%d m=%d", B.kmax, B.mmax); return SPG_ECAPACITY; }
            B.gws_stride = ((size_t)L.mat_doubles + 31) & ~(size_t)31;
            continue;
        }
        // latency mode: a launch that cannot fill the chip (<= 2 blankets per CU) gives every blanket
        // two wavefronts so the Chow-Liu and gauge chains overlap; throughput mode keeps one
        const bool two_waves = nfr && nb <= 512 && D * B.kmax <= spgdev::kWaveMax && !cfg.force_one_wave;
        // tiles beyond the register-resident size (n > 24) run the LDS-cooperative routines: their O(n^2) inner
        // steps want lanes, and a launch this small leaves the chip empty anyway — four wavefronts per blanket
        // (parking.g2o: 0.70 -> ms per launch of such blankets)
        const bool four_waves = !two_waves && nfr && !lm && nb <= 1024 && D * B.kmax > spgdev::kWaveMax && !cfg.force_one_wave;
        const int nt = two_waves ? 128 : four_waves ? 256 : 64;
        const Layout L = layout(nt);
        B.variant = {D, nt, false, alg};
        // the (kmax, mmax, smax) envelope can exceed the device limit although every member fits
        // (each needs <= lim[i] <= lds_limit): clamp, the per-block carve-up uses its own k, m
        B.lds = std::min((size_t)(L.small_doubles + L.mat_doubles) * 8, (size_t)cfg.lds_limit);
    }
    return 0;
}

// The launch path of a round: bins, generic list, big list, variants. 0 or SPG_ECAPACITY with its text in err.
inline int plan_launch(const spg_round_desc *rd, const PlanConfig &cfg, RoundPlan &P, char *err, size_t errlen) {
    for (PlanBin &B : P.bins) { B.list.clear(); B.kmax = B.mmax = B.smax = 0; B.bytes = 0; B.lds = B.gws_stride = 0; }
    P.ip_list.clear(); P.big_list.clear();
    P.ip_closed = 0; P.ip_stride = P.ip_hot = 0;
    plan_bins(rd, cfg, P);
    if (int rc = plan_generic(rd, cfg, P, err, errlen)) return rc;
    if (int rc = plan_big(rd, cfg, P, err, errlen)) return rc;
    return plan_variants(rd, cfg, P, err, errlen);
}

// The launch lists as the kernels read them, back to back: bins 0..4, then the generic list (together never more than
// the round's count). Returns the number of entries written.
inline size_t staged_list(const RoundPlan &P, int32_t *lst) {
    size_t p = 0;
    for (const PlanBin &B : P.bins) for (int32_t b : B.list) lst[p++] = b;
    for (int32_t b : P.ip_list) lst[p++] = b;
    return p;
}

inline int plan_round(const spg_round_desc *rd, const PlanConfig &cfg, const WorkerState &ws, RoundPlan &P, char *err, size_t errlen) {
    plan_worker(rd, cfg, ws, P);
    return P.to_worker ? 0 : plan_launch(rd, cfg, P, err, errlen);
}

}  // namespace spg
#pragma GCC visibility pop
