// csrc/spg_kernels.hip — the per-blanket marginalisation kernels for gfx950 and their launch entry points
// (the HIP backend that plans and launches one conflict-free round of blankets is host code: spg_hip_backend.cpp).
//
// One workgroup per Markov blanket (64 lanes = one wavefront for blankets whose tiles fit in LDS,
// 256 lanes with an L2-resident workspace for the rare large ones). The whole per-vertex iteration
// of the reference's VertexRemover::remove (src/vertex_remover.cpp:108-132) runs inside the kernel:
//
//   gather     poses + edge records of the blanket straight from the HBM-resident arena
//   assemble   H = sum_e J_e^T Omega_e J_e                   (g2o buildSystem, src/vertex_remover.cpp:397-402)
//   Schur      Lambda_t = H_kk - H_mk^T LLT(H_mm)^-1 H_mk    (src/vertex_remover.cpp:444-449)
//   topology   pseudo-Chow-Liu: (Lambda_t + I)^-1, pairwise log-det weights, Kruskal
//                                                             (src/pseudo_chow_liu.cpp:33-87,169-196,253-289)
//   skeleton   z_ab = x_a^-1 x_b, Jacobians at zero error     (src/topology_provider_binary.hpp:40-47,
//                                                              src/vertex_remover.cpp:466-498)
//   recover    eig(Lambda_t), gauge drop, Sigma = U S U^T, X_e = (J_e Sigma J_e^T)^-1
//                                                             (src/logdet_function.cpp:14-64,236-279)
//   KLD        1/2 (tr(S M) - logdet M - logdet S - r), M = U^T (J^T X J) U
//                                                             (src/logdet_function.cpp:119-133,281-323)
//   scatter    new edge records + per-blanket output record back into the arena
//
// 3x3 / 6x6 information blocks, Jacobians and the n x n tiles (n = d*k) live in LDS; HBM traffic is
// the algorithmic minimum: every pose and edge record is read once, every new record written once.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdio>
#include "../../include/spg.h"
#include "spg_blanket_layout.hpp"
#include "spg_dev_geom.hpp"
#include "spg_dev_la.hpp"
#include "spg_dev_wave.hpp"
#include "spg_internal.h"

using namespace spgdev;

using spg::EC; using spg::SPG_ALG_NFR_LM; using spg::Layout; using spg::make_layout; using spg::KArgs;

namespace {

// A value every lane holds identically: pin it to scalar registers. The descriptor fields steer every loop bound and
// tile offset of a blanket; where they arrive through LDS or a stack slot (persistent worker) the compiler would
// otherwise carry them — and everything derived from them — in vector registers.
__device__ __forceinline__ int uni32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned long long uni64(unsigned long long v) {
    unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(v & 0xffffffffu)), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (unsigned long long)lo | ((unsigned long long)hi << 32);
}
template <class T>
__device__ __forceinline__ T *uniptr(T *p) { return reinterpret_cast<T *>(uni64(reinterpret_cast<unsigned long long>(p))); }

// upper-triangular (row-wise) index of (r,c), r <= c
__device__ __forceinline__ int utri(int r, int c, int D) { return r * D - (r * (r - 1)) / 2 + (c - r); }

// One blanket on one workgroup of NT lanes. bd = its descriptor; bvpo[0..n_vert) the arena offsets of its poses,
// ber[0..n_edge) its edge references (vbegin indexes bev[]); gws_slot = index of the workgroup's global workspace.
// Called by blanket_kernel (one launch per batch, descriptors in global memory) and by blanket_worker (persistent
// workgroups fed through a queue, descriptors staged in LDS).
// Edge records written by OTHER workgroups of the same kernel (persistent worker: the new edges of earlier blankets)
// are read with agent-scope loads: each XCD has its own L2, and a line that holds a neighbouring, earlier record may
// already sit there stale. Launched kernels read them plainly (a kernel boundary lies between writer and reader).
template <bool COH>
__device__ __forceinline__ double ldrec(const double *p) {
    if (COH) return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return *p;
}

// ... and written with system-scope (write-through) stores there: the ready word may then follow after a plain
// s_waitcnt instead of a system-scope release fence, which writes back every dirty line of the XCD's L2 (measured:
// publish() 11.7k cycles of a 90k-cycle blanket with the fence).
template <bool COH>
__device__ __forceinline__ void strec(double *p, double v) {
    if (COH) __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else *p = v;
}
__device__ __forceinline__ void wait_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---- gauge route, shared by the NFR information recovery and the GLC per-blanket KLD (SPG_FLAG_GLC_KLD)
// Lambda_t of a blanket of relative measurements has an exactly known d-dimensional null space: the rigid motions of the
// whole blanket, N = [G_1; ...; G_k] in the vertices' update coordinates. kpose = the kept vertices' poses (LDS form).
template <int D, class TeamT>
__device__ __forceinline__ void gauge_basis_raw(const TeamT TT, const double *kpose, int k, double *Ng) {
    constexpr int DD = D * D, PSZ = (D == 6) ? 12 : 3;
    for (int v = TT.tid; v < k; v += TT.size) {
        const double *X = kpose + v * PSZ;
        double *Gv = Ng + v * DD;
        if (D == 6) {
#pragma unroll
            for (int rr = 0; rr < 3; rr++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    // R^T ; -R^T [t]x ; 0 ; 1/2 R^T   (column c of [t]x is t x e_c)
                    constexpr int A1[3] = {1, 2, 0}, B1[3] = {2, 0, 1};
                    const int ca = A1[c], cb = B1[c];
                    double rt = X[c * 3 + rr];
                    // (t x e_c): component cb = +t[ca]... derive: t x e_c = (t_a e_a + t_b e_b + t_c e_c) x e_c
                    //   e_a x e_c = -e_b , e_b x e_c = +e_a   (a = c+1, b = c+2 cyclic)
                    //   => t x e_c = t_b e_a - t_a e_b
                    double cx_a = X[9 + cb], cx_b = -X[9 + ca];
                    double val = -(X[ca * 3 + rr] * cx_a + X[cb * 3 + rr] * cx_b);  // -(R^T (t x e_c))[rr]
                    Gv[rr * 6 + c] = rt;
                    Gv[rr * 6 + 3 + c] = val;
                    Gv[(3 + rr) * 6 + c] = 0.0;
                    Gv[(3 + rr) * 6 + 3 + c] = 0.5 * rt;
                }
        } else {
            Gv[0] = 1; Gv[1] = 0; Gv[2] = -X[1];
            Gv[3] = 0; Gv[4] = 1; Gv[5] = X[0];
            Gv[6] = 0; Gv[7] = 0; Gv[8] = 1;
        }
    }
    TT.sync();
}
// orthonormalise: N^ = N L^-T with N^T N = L L^T (D x D, one lane, registers). scr: 2 D^2 doubles. Sets *TT.flag on failure.
template <int D, class TeamT>
__device__ __forceinline__ void gauge_orthonormalise(const TeamT TT, int n, double *Ng, double *scr) {
    constexpr int DD = D * D;
    if (TT.tid < DD) {
        int rr = TT.tid / D, c = TT.tid - rr * D;
        double s = 0;
        for (int i = 0; i < n; i++) s += Ng[i * D + rr] * Ng[i * D + c];
        scr[TT.tid] = s;
    }
    TT.sync();
    if (TT.tid == 0) {
        double Ab[DD], Li[DD];
#pragma unroll
        for (int i = 0; i < DD; i++) Ab[i] = scr[i];
        if (!chol_reg<D>(Ab)) (*TT.flag) = 1;
#pragma unroll
        for (int c = 0; c < D; c++)
#pragma unroll
            for (int i = 0; i < D; i++) {
                if (i < c) Li[i * D + c] = 0.0;
                else if (i == c) Li[i * D + c] = 1.0 / Ab[c * D + c];
                else {
                    double s = 0;
#pragma unroll
                    for (int q = 0; q < D; q++) if (q >= c && q < i) s += Ab[i * D + q] * Li[q * D + c];
                    Li[i * D + c] = -s / Ab[i * D + i];
                }
            }
#pragma unroll
        for (int i = 0; i < DD; i++) scr[DD + i] = Li[i];
    }
    TT.sync();
    {
        double nv_[D];
        for (int i = TT.tid; i < n; i += TT.size) {
#pragma unroll
            for (int c = 0; c < D; c++) {
                double s = 0;
#pragma unroll
                for (int q = 0; q < D; q++) if (q <= c) s += Ng[i * D + q] * scr[DD + c * D + q];
                nv_[c] = s;
            }
#pragma unroll
            for (int c = 0; c < D; c++) Ng[i * D + c] = nv_[c];
        }
    }
    TT.sync();
}
// C = Lam + N^ N^^T (full symmetric) into Cm; Lam's lower triangle is read
template <int D, class TeamT>
__device__ __forceinline__ void gauge_regularised(const TeamT TT, const double *Lam, int ld, int n, const double *Ng, double *Cm) {
    int sh = ceil_log2(n), tot = n << sh;
    for (int it = TT.tid; it < tot; it += TT.size) {
        int i = it >> sh, j = it & ((1 << sh) - 1);
        if (j <= i) {
            double s = Lam[i * ld + j];
#pragma unroll
            for (int q = 0; q < D; q++) s += Ng[i * D + q] * Ng[j * D + q];
            Cm[i * ld + j] = s;
            Cm[j * ld + i] = s;
        }
    }
    TT.sync();
}
// Am += N^ N^^T, every entry
template <int D, class TeamT>
__device__ __forceinline__ void gauge_add(const TeamT TT, double *Am, int ld, int n, const double *Ng) {
    int sh = ceil_log2(n), tot = n << sh;
    for (int it = TT.tid; it < tot; it += TT.size) {
        int i = it >> sh, j = it & ((1 << sh) - 1);
        if (j < n) {
            double s = 0;
#pragma unroll
            for (int q = 0; q < D; q++) s += Ng[i * D + q] * Ng[j * D + q];
            Am[i * ld + j] += s;
        }
    }
    TT.sync();
}

template <int D, int NT, bool GWS, int ALG, bool COH = false>
__device__ __forceinline__ void blanket_body(const KArgs &a_in, const spg_blanket_desc &bd_in, const int64_t *bvpo_in, const spg_edge_ref *ber_in,
                                             const int32_t *bev_in, const int gws_slot, double *smem) {
    KArgs a;
    a.arena = uniptr(a_in.arena); a.gws = uniptr(a_in.gws); a.mail = uniptr(a_in.mail);
    a.gws_stride = (int64_t)uni64((unsigned long long)a_in.gws_stride); a.mail_base = (int64_t)uni64((unsigned long long)a_in.mail_base);
    a.topology = uni32(a_in.topology); a.algorithm = uni32(a_in.algorithm); a.flags = uni32(a_in.flags);
    a.lin_point = uni32(a_in.lin_point); a.tag = uni32(a_in.tag);
    a.chord_ratio = __longlong_as_double((long long)uni64((unsigned long long)__double_as_longlong(a_in.chord_ratio)));
    a.blk = nullptr; a.vpo = nullptr; a.er = nullptr; a.ev = nullptr; a.list = nullptr;
    spg_blanket_desc bd;
    bd.vert_begin = 0; bd.edge_begin = 0; bd.new_len = 0;
    bd.n_vert = uni32(bd_in.n_vert); bd.n_remove = uni32(bd_in.n_remove); bd.n_edge = uni32(bd_in.n_edge);
    bd.n_new_max = uni32(bd_in.n_new_max); bd.n_new_vert_max = uni32(bd_in.n_new_vert_max); bd.pad_ = uni32(bd_in.pad_);
    bd.new_off = (int64_t)uni64((unsigned long long)bd_in.new_off); bd.out_off = (int64_t)uni64((unsigned long long)bd_in.out_off);
    bd.tinfo_off = (int64_t)uni64((unsigned long long)bd_in.tinfo_off);
    const int64_t *bvpo = uniptr(bvpo_in);
    const spg_edge_ref *ber = uniptr(ber_in);
    const int32_t *bev = uniptr(bev_in);
    constexpr int DD = D * D;
    constexpr int PS = (D == 6) ? 7 : 3;    // pose / measurement doubles in the arena
    constexpr int PSZ = (D == 6) ? 12 : 3;  // pose doubles in LDS
    constexpr int REC = PS + D * (D + 1) / 2;
    const int tid = threadIdx.x;
    const int nv = bd.n_vert, m = bd.n_remove, k = nv - m;
    const Layout L = make_layout(D, NT, k, m, ALG, a.topology, bd.pad_);
    const int n = L.n, nm = L.nm, ld = L.ld, ldm = L.ldm;
    double *mat = GWS ? (a.gws + (size_t)gws_slot * (size_t)a.gws_stride) : (smem + L.small_doubles);
    double *pose = smem + L.o_pose, *cs = smem + L.o_cs, *ev = smem + L.o_ev, *Sv = smem + L.o_S;
    double *w = smem + L.o_w, *ldb = smem + L.o_ldb, *Lb = smem + L.o_Lb, *nJ = smem + L.o_nJ, *X = smem + L.o_X;
    double *eJ = smem + L.o_eJ, *eO = smem + L.o_eO, *eT = smem + L.o_eT;
    int *ints = reinterpret_cast<int *>(smem + L.o_int);
    int *perm = ints + L.i_perm, *keep = ints + L.i_keep, *sorted = ints + L.i_sorted, *comp = ints + L.i_comp;
    int *pairs = ints + L.i_pairs, *echv = ints + L.i_ev, *misc = ints + L.i_misc, *pij = ints + L.i_pij;
    double *M1 = mat + L.o_M1, *M2 = mat + L.o_M2, *M3 = mat + L.o_M3, *Hmm = mat + L.o_Hmm, *Hmk = mat + L.o_Hmk;
    Team<NT> T{tid, smem + L.o_red, misc + 0};
    // register-resident single-wavefront SPD kernels (spg_dev_wave.hpp) when the tile fits
    const bool use_wave_hw = !GWS && (n <= kWaveMax) && !((a.flags >> 17) & 1);
    const bool use_wave = use_wave_hw && (NT == 64);
    // two wavefronts per blanket: the Chow-Liu chain and the gauge chain run side by side (NFR only)
    const bool split = (NT == 128) && (ALG != SPG_ALG_GLC) && use_wave_hw && !(a.flags & SPG_FLAG_FORCE_EIG);
    double *xch = smem + L.o_xch;
    double *arena = a.arena;
    double *orec = a.mail ? (a.mail + (bd.out_off - a.mail_base)) : (arena + bd.out_off);

    int status = SPG_OK, info = 0, n_new = 0;
    double kld = __builtin_nan(""), min_gap = __builtin_inf();

    // publish(): everything the host's graph update needs — status so far, n_new, the new-edge table —
    // followed by a system-scope release and the ready tag. finish() = publish (unless done) + KLD.
    bool published = false;
    // Worker (COH): the new edge records and the out record are staged in LDS (recbuf / orl) and leave as a few
    // coalesced write-through stores — one word per lane — instead of ~110 single stores by the lanes that compute them:
    // a system-scope store is acknowledged over the fabric (PCIe for the mailbox), and a lane that issues them one by one
    // pays that round trip per store.
    double *recbuf = smem + L.o_eJ;     // ne x REC doubles (eJ is free after the assembly)
    double *orl = smem + L.o_eO;        // the out record (<= 6 + 4 k + 2 k doubles; eO is free after the assembly)
    auto publish = [&]() {
        if (COH) {
            T.sync();   // recbuf is complete
            const int nrec = n_new * REC;
            for (int it = tid; it < nrec; it += NT) strec<true>(arena + bd.new_off + it, recbuf[it]);
            // compact out record (streaming driver, flags bit 20): ONE cache line — the six header words, then the new edges'
            // endpoint pairs as local vertex indices, 4 bits each, edge e in byte e of words [6] (e < 8) and [7]; the edge
            // table is implied (pose-pose records of REC doubles, back to back at new_off). The host polls, reads and later
            // re-reads (KLD, final word) a single line per blanket instead of five.
            const bool compact = (a.flags >> 20) & 1;
            if (tid == 0) {
                orl[0] = (double)status; orl[1] = (double)info; orl[2] = kld; orl[3] = min_gap; orl[4] = (double)n_new; orl[5] = 0.0;
                if (compact) {
                    unsigned long long w0 = 0, w1 = 0;
                    for (int e = 0; e < n_new; e++) {
                        const unsigned long long pr = (unsigned long long)((m + pairs[2 * e]) & 15) | ((unsigned long long)((m + pairs[2 * e + 1]) & 15) << 4);
                        if (e < 8) w0 |= pr << (8 * e); else w1 |= pr << (8 * (e - 8));
                    }
                    orl[6] = __longlong_as_double((long long)w0); orl[7] = __longlong_as_double((long long)w1);
                } else
                for (int e = 0; e < n_new; e++) {
                    orl[SPG_OUT_HDR + 4 * e + 0] = (double)SPG_EDGE_BINARY;
                    orl[SPG_OUT_HDR + 4 * e + 1] = (double)(e * REC);
                    orl[SPG_OUT_HDR + 4 * e + 2] = (double)REC;
                    orl[SPG_OUT_HDR + 4 * e + 3] = 2.0;
                    orl[SPG_OUT_HDR + 4 * bd.n_new_max + 2 * e + 0] = (double)(m + pairs[2 * e]);
                    orl[SPG_OUT_HDR + 4 * bd.n_new_max + 2 * e + 1] = (double)(m + pairs[2 * e + 1]);
                }
            }
            wait_stores();   // this lane's record stores have been acknowledged
            T.sync();        // ... everybody's; orl is complete
            const int olen = compact ? 8 : SPG_OUT_HDR + 4 * bd.n_new_max + 2 * n_new;
            if (tid < 64) {   // (wave 0; olen <= 42 for the blankets a worker takes)
                for (int t = tid; t < olen; t += 64) if (t != 5) strec<true>(orec + t, orl[t]);
                wait_stores();   // wave 0's stores are out before its lane 0 raises the ready word
                if (tid == 0) {
                    __hip_atomic_store(&orec[5], SPG_READY_WORD(a.tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    orl[5] = (double)wall_clock64();   // (SPG_WORKER_STAMP diagnostics: when the ready word left)
                }
            }
            published = true;
            return;
        }
        T.sync();  // every lane's new-record stores precede the release below
        if (tid == 0) {
            orec[0] = (double)status; orec[1] = (double)info; orec[2] = kld; orec[3] = min_gap; orec[4] = (double)n_new;
            for (int e = 0; e < n_new; e++) {
                orec[SPG_OUT_HDR + 4 * e + 0] = (double)SPG_EDGE_BINARY;
                orec[SPG_OUT_HDR + 4 * e + 1] = (double)(e * REC);
                orec[SPG_OUT_HDR + 4 * e + 2] = (double)REC;
                orec[SPG_OUT_HDR + 4 * e + 3] = 2.0;
                orec[SPG_OUT_HDR + 4 * bd.n_new_max + 2 * e + 0] = (double)(m + pairs[2 * e]);
                orec[SPG_OUT_HDR + 4 * bd.n_new_max + 2 * e + 1] = (double)(m + pairs[2 * e + 1]);
            }
        }
        __threadfence_system();
        T.sync();
        if (tid == 0) {
            __hip_atomic_store(&orec[5], SPG_READY_WORD(a.tag), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        published = true;
    };
    auto finish = [&]() {
        if (!published) publish();
        else if (tid == 0) { strec<COH>(orec + 2, kld); strec<COH>(orec + 0, (double)status); }
        // the record is complete (KLD and a possible SPG_ST_KLD_NOT_PD included): final word, after a release
        if (tid == 0) {
            if (COH) { wait_stores(); __hip_atomic_store(&orec[5], SPG_FINAL_WORD(a.tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
            else { __threadfence_system(); __hip_atomic_store(&orec[5], SPG_FINAL_WORD(a.tag), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
        }
    };
    // diagnostic cycle stamps (flags bit 16, needs tinfo_off >= 0): written only to the debug region
    const bool stamping = ((a.flags >> 16) & 1) && bd.tinfo_off >= 0;
    auto STAMP = [&](int idx) {
        if (stamping) {
            T.sync();
            if (tid == 0) arena[bd.tinfo_off + idx] = (double)__builtin_amdgcn_s_memtime();
        }
    };
    // inside the two concurrent chains of the two-wavefront variant: no workgroup barrier, lane 0 of each wave stamps
    auto CSTAMP = [&](int idx) {
        if (stamping) {
            if (!split) { T.sync(); if (tid == 0) arena[bd.tinfo_off + idx] = (double)__builtin_amdgcn_s_memtime(); }
            else if ((tid & 63) == 0) arena[bd.tinfo_off + idx] = (double)__builtin_amdgcn_s_memtime();
        }
    };
    STAMP(0);  //
    // ---------------------------------------------------------------- gather poses, clear H
    if (tid == 0) { misc[0] = 0; misc[1] = 0; misc[2] = 0; misc[6] = 0; misc[7] = 0; misc[8] = 0; misc[9] = 0; }
    for (int v = tid; v < nv; v += NT) {
        const double *p = arena + bvpo[v];
        if (D == 6) iso_from_tq(p, pose + v * PSZ);
        else { pose[v * PSZ] = p[0]; pose[v * PSZ + 1] = p[1]; pose[v * PSZ + 2] = p[2]; }
    }
    for (int i = tid; i < n * ld; i += NT) M1[i] = 0.0;
    for (int i = tid; i < nm * ldm; i += NT) Hmm[i] = 0.0;
    for (int i = tid; i < nm * ld; i += NT) Hmk[i] = 0.0;
    T.sync();
    STAMP(23);  // gathered + cleared
    if (bd.n_edge == 0 || m < 1) { status = SPG_ST_EMPTY_BLANKET; finish(); return; }
    constexpr bool is_glc = (ALG == SPG_ALG_GLC);  // compile-time: the NFR instantiation carries no GLC code
    constexpr bool has_lm = (ALG == SPG_ALG_NFR_LM);
    if (is_glc && !(a.topology == SPG_TOPO_DENSE || a.topology == SPG_TOPO_TREE)) {
        status = SPG_ST_UNSUPPORTED;  // asserts at src/topology_provider_glc.cpp:107-111
        finish(); return;
    }

    // Local linearisation point without a closed form: lm_left LM iterations on the blanket (below)
    int lm_left = 0;
    // (a cluster with fewer than two kept vertices emits no edge whatever the linearisation point: it is not re-linearised;
    //  clusters with k >= 2 under Local go to the generic kernel behind the pre-pass of hip_run_round)
    if (a.lin_point != SPG_LIN_GLOBAL && !(m > 1 && k < 2)) {
        // Local linearisation point, closed-form branch of buildSubgraph (src/vertex_remover.cpp:304-381):
        // possible iff every vertex but the first removed one sits in exactly one (pose-pose) blanket edge;
        // then the removed vertex goes to the origin and each neighbour to z (or z^-1) of its edge.
        if (is_glc) { status = SPG_ST_UNSUPPORTED; finish(); return; }  // src/topology_provider_glc.cpp:110-111
        // the per-vertex edge counters below live in perm[] (n ints): a cluster with many removed and few kept vertices
        // (n < nv) would write past it, and clusters under a Local point are not built anyway — leave before any write
        if (n < nv || m != 1) { status = SPG_ST_NEEDS_LOCAL_OPTIMIZATION; finish(); return; }
        int *cntv = perm;
        for (int v = tid; v < nv; v += NT) cntv[v] = 0;
        T.sync();
        for (int e = tid; e < bd.n_edge; e += NT) {
            const spg_edge_ref er = ber[e];
            if (er.kind != SPG_EDGE_BINARY) { misc[8] = 1; continue; }
            int vi = bev[er.vbegin], vj = bev[er.vbegin + 1];
            if (vi != 0) atomicAdd(&cntv[vi], 1);
            if (vj != 0) atomicAdd(&cntv[vj], 1);
        }
        T.sync();
        for (int v = 1 + tid; v < nv; v += NT) if (cntv[v] > 1) misc[9] = 1;
        T.sync();
        // a GLC edge cannot propagate an estimate, and clusters (m > 1) with a Local point are not built
        if (misc[8] || n < nv || (misc[9] && m != 1)) { status = SPG_ST_NEEDS_LOCAL_OPTIMIZATION; finish(); return; }
        if (misc[9]) {
            // some kept vertex sits in several blanket edges: the reference fixes the removed vertex at its
            // current estimate and runs 10 LM iterations on the subgraph (src/vertex_remover.cpp:382-391)
            if constexpr (has_lm) lm_left = 10;
            else { status = SPG_ST_NEEDS_LOCAL_OPTIMIZATION; finish(); return; }   // (the host launches the LM variant for Local)
        } else {
        if (tid == 0) {
            if (D == 6) {
#pragma unroll
                for (int t_ = 0; t_ < kIso; t_++) pose[t_] = (t_ == 0 || t_ == 4 || t_ == 8) ? 1.0 : 0.0;
            }
            else { pose[0] = 0; pose[1] = 0; pose[2] = 0; }
        }
        for (int e = tid; e < bd.n_edge; e += NT) {
            const spg_edge_ref er = ber[e];
            int vi = bev[er.vbegin], vj = bev[er.vbegin + 1];
            const double *rec = arena + er.off;
            if (vi == 0 && vj == 0) continue;
            if (D == 6) {
                double Z[kIso];
                iso_from_tq(rec, Z);
                if (vi == 0) {
#pragma unroll
                    for (int t_ = 0; t_ < kIso; t_++) pose[vj * PSZ + t_] = Z[t_];
                }
                else {
                    double I12[kIso] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, Zi[kIso];
                    iso_inv_mul(Z, I12, Zi);
#pragma unroll
                    for (int t_ = 0; t_ < kIso; t_++) pose[vi * PSZ + t_] = Zi[t_];
                }
            } else {
                if (vi == 0) { pose[vj * PSZ] = rec[0]; pose[vj * PSZ + 1] = rec[1]; pose[vj * PSZ + 2] = normalize_theta(rec[2]); }
                else {
                    double c = cos(rec[2]), sn = sin(rec[2]);
                    pose[vi * PSZ] = -(c * rec[0] + sn * rec[1]);
                    pose[vi * PSZ + 1] = -(-sn * rec[0] + c * rec[1]);
                    pose[vi * PSZ + 2] = normalize_theta(-rec[2]);
                }
            }
        }
        }
        T.sync();
    }
    // ---------------------------------------------------------------- assemble H (a6)
    auto hadd = [&](int R, int Cc, double val) {
        if (R < nm) {
            if (Cc < nm) Hmm[R * ldm + Cc] += val;
            else Hmk[R * ld + (Cc - nm)] += val;
        } else if (Cc >= nm) {
            M1[(R - nm) * ld + (Cc - nm)] += val;
        }
    };
    // LM state (uniform over the workgroup; only used when lm_left > 0). The system of an LM iteration is
    // what the assembly produces anyway: H = M1 (kept block: the removed vertex is fixed), plus the
    // right-hand side b = -sum J^T Omega e and chi2, which the assembly adds in LM mode. M2 / Sv keep the
    // system of the last accepted estimates, M3 takes the factorisation, Ng the backup of the estimates.
    double *eE = nJ;                      // errors of the staged edges (EC x D)
    double *bnew = ev, *bcur = Sv, *xs = cs, *pbak = smem + L.o_Ng;
    double lm_lambda = 0, lm_ni = 2, lm_chi = 0, lm_scale = 0;
    int lm_it = 0, lm_q = 0, lm_phase = 0;
    bool lm_redo = false;                 // the tiles hold a rejected trial: assemble once more, then go on
    for (;;) {
    if (has_lm && (lm_left > 0 || lm_redo)) {
        if (lm_phase > 0 || lm_redo) {
            for (int i = tid; i < n * ld; i += NT) M1[i] = 0.0;
            for (int i = tid; i < nm * ldm; i += NT) Hmm[i] = 0.0;
            for (int i = tid; i < nm * ld; i += NT) Hmk[i] = 0.0;
        }
        for (int i = tid; i < n; i += NT) bnew[i] = 0.0;
        if (tid == 0) xch[0] = 0.0;
        T.sync();
    }
    for (int base = 0; base < bd.n_edge; base += EC) {
        int cnt = min(EC, bd.n_edge - base);
        if (tid < cnt) {
            const spg_edge_ref er = ber[base + tid];
            int vi = 0, vj = 0;
            if (er.kind == SPG_EDGE_BINARY) {
                vi = bev[er.vbegin]; vj = bev[er.vbegin + 1];
                double rec[PS];
#pragma unroll
                for (int i = 0; i < PS; i++) rec[i] = ldrec<COH>(arena + er.off + i);
                if (D == 6) {
                    double Z[kIso];
                    iso_from_tq(rec, Z);
                    se3_edge_jac(pose + vi * PSZ, pose + vj * PSZ, Z, eJ + tid * 2 * DD, eJ + tid * 2 * DD + DD, (has_lm && lm_left > 0) ? eE + tid * D : nullptr);
                } else {
                    se2_edge_jac(pose + vi * PSZ, pose + vj * PSZ, rec, eJ + tid * 2 * DD, eJ + tid * 2 * DD + DD, (has_lm && lm_left > 0) ? eE + tid * D : nullptr);
                }
            } else {
                if (!is_glc) misc[1] = 1;  // GLC edge inside an NFR blanket: no provider applies
                vi = -1;                    // handled by the n-ary loop below
            }
            echv[2 * tid] = vi; echv[2 * tid + 1] = vj;
        }
        for (int it = tid; it < cnt * DD; it += NT) {
            int e = it / DD, rc = it - e * DD, r = rc / D, c = rc - r * D;
            const spg_edge_ref er = ber[base + e];
            int lo = r < c ? r : c, hi = r < c ? c : r;
            eO[it] = (er.kind == SPG_EDGE_BINARY) ? ldrec<COH>(arena + er.off + PS + utri(lo, hi, D)) : 0.0;
        }
        T.sync();
        STAMP(24);  // jacobians + omega staged
        // T_e = Omega_e [Ji | Jj] for every staged edge at once
        for (int it = tid; it < cnt * 2 * DD; it += NT) {
            int e = it / (2 * DD), rem = it - e * 2 * DD, wch = rem / DD, rc = rem - wch * DD, r = rc / D, c = rc - r * D;
            const double *J = eJ + e * 2 * DD + wch * DD, *Om = eO + e * DD;
            double s = 0;
#pragma unroll
            for (int p = 0; p < D; p++) s += Om[r * D + p] * J[p * D + c];
            eT[it] = s;
        }
        T.sync();
        STAMP(25);  // T = Omega J
        if (has_lm && lm_left > 0) {
            // LM mode: b_v -= (Omega J_v)^T e and chi2 += e^T Omega e. Lanes own (edge, side, row); the edges
            // of the chunk are folded in serially so that the sums keep a fixed order.
            {
                double c2 = 0;
                for (int it = tid; it < cnt * D; it += NT) {
                    int e = it / D, p = it - e * D;
                    if (echv[2 * e] < 0) continue;
                    const double *Om = eO + e * DD, *er_ = eE + e * D;
                    double sacc = 0;
#pragma unroll
                    for (int q = 0; q < D; q++) sacc += Om[p * D + q] * er_[q];
                    c2 += er_[p] * sacc;
                }
                c2 = T.sum(c2);
                if (tid == 0) xch[0] += c2;
                for (int e = 0; e < cnt; e++) {
                    if (echv[2 * e] < 0) continue;   // (uniform: echv is shared)
                    for (int side = 0; side < 2; side++) {
                        const int v = echv[2 * e + side];
                        if (tid < D && v >= 1) {     // the removed vertex (local 0, m == 1) is fixed
                            const double *Te = eT + e * 2 * DD + side * DD, *er_ = eE + e * D;
                            double sacc = 0;
#pragma unroll
                            for (int p = 0; p < D; p++) sacc += Te[p * D + tid] * er_[p];
                            bnew[(v - 1) * D + tid] -= sacc;
                        }
                        T.sync();
                    }
                }
            }
            T.sync();
        }
        if (NT == 64) {
            // One wavefront: LDS atomics retire in program order and every ds_add_f64 below carries the
            // items of a single edge (128-slot stride, 108 used), so no two lanes of one instruction hit
            // the same address and contributions land in ascending edge order — deterministic, without a
            // barrier per edge.
            auto hadd_atomic = [&](int R, int Cc, double val) {
                double *dst = nullptr;
                if (R < nm) dst = (Cc < nm) ? &Hmm[R * ldm + Cc] : &Hmk[R * ld + (Cc - nm)];
                else if (Cc >= nm) dst = &M1[(R - nm) * ld + (Cc - nm)];
                if (dst) __hip_atomic_fetch_add(dst, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            };
            constexpr int SLOT = (3 * DD + 63) / 64 * 64;
            for (int it = tid; it < cnt * SLOT; it += NT) {
                int e = it / SLOT, loc = it - e * SLOT;
                if (loc >= 3 * DD || echv[2 * e] < 0) continue;
                const double *Ji = eJ + e * 2 * DD, *Jj = Ji + DD, *Te = eT + e * 2 * DD;
                int vi = echv[2 * e], vj = echv[2 * e + 1];
                int blk = loc / DD, rc = loc - blk * DD, r = rc / D, c = rc - r * D;
                const double *Ja = (blk == 2) ? Jj : Ji;
                const double *Tb = (blk == 0) ? Te : Te + DD;
                double s = 0;
#pragma unroll
                for (int p = 0; p < D; p++) s += Ja[p * D + r] * Tb[p * D + c];
                if (blk == 0) hadd_atomic(vi * D + r, vi * D + c, s);
                else if (blk == 2) hadd_atomic(vj * D + r, vj * D + c, s);
                else if (vi != vj) {
                    hadd_atomic(vi * D + r, vj * D + c, s);
                    hadd_atomic(vj * D + c, vi * D + r, s);
                }
            }
            T.sync();
        } else {
        // accumulate edge by edge (blocks of different edges overlap on the shared vertices)
        for (int e = 0; e < cnt; e++) {
            if (echv[2 * e] < 0) continue;
            const double *Ji = eJ + e * 2 * DD, *Jj = Ji + DD, *Te = eT + e * 2 * DD;
            int vi = echv[2 * e], vj = echv[2 * e + 1];
            for (int it = tid; it < 3 * DD; it += NT) {
                int blk = it / DD, rc = it - blk * DD, r = rc / D, c = rc - r * D;
                const double *Ja = (blk == 2) ? Jj : Ji;
                const double *Tb = (blk == 0) ? Te : Te + DD;
                double s = 0;
#pragma unroll
                for (int p = 0; p < D; p++) s += Ja[p * D + r] * Tb[p * D + c];
                if (blk == 0) hadd(vi * D + r, vi * D + c, s);
                else if (blk == 2) hadd(vj * D + r, vj * D + c, s);
                else if (vi != vj) { hadd(vi * D + r, vj * D + c, s); hadd(vj * D + c, vi * D + r, s); }
            }
            T.sync();
        }
        }
    }
    if (!has_lm || lm_redo || lm_left <= 0) break;   // ordinary case: one assembly
    if constexpr (has_lm)
    // ---- g2o Levenberg-Marquardt on the blanket, removed vertex fixed (OptimizationAlgorithmLevenberg:
    //      lambda_0 = 1e-5 max diag, <= 10 trials per iteration, rho = (chi2 - chi2') / (x.(lambda x + b) + 1e-3),
    //      good step: lambda *= clamp(1 - (2 rho - 1)^3, 1/3, 2/3); bad step: lambda *= ni, ni *= 2)
    {
        const double chi_new = xch[0];
        bool next_trial = false, done = false;
        if (lm_phase == 0) {
            // first system: the current estimates
            lm_chi = chi_new;
            if (tid == 0) { double md = 0; for (int i = 0; i < n; i++) md = fmax(md, fabs(M1[i * ld + i])); xch[1] = md; }
            T.sync();
            lm_lambda = 1e-5 * xch[1];
            lm_ni = 2; lm_it = 0; lm_q = 0;
            for (int i = tid; i < n * ld; i += NT) M2[i] = M1[i];
            for (int i = tid; i < n; i += NT) bcur[i] = bnew[i];
            T.sync();
            lm_phase = 1;
            next_trial = true;
        } else {
            const double rho = (lm_chi - chi_new) / (lm_scale + 1e-3);
            if (rho > 0 && isfinite(chi_new)) {
                double alpha = 1.0 - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1);
                alpha = fmin(alpha, 2.0 / 3.0);
                lm_lambda *= fmax(1.0 / 3.0, alpha);
                lm_ni = 2;
                lm_chi = chi_new;
                for (int i = tid; i < n * ld; i += NT) M2[i] = M1[i];
                for (int i = tid; i < n; i += NT) bcur[i] = bnew[i];
                T.sync();
                lm_it++; lm_q = 0;
                if (lm_it >= lm_left) done = true;          // the tiles hold the system of the accepted estimates
                else next_trial = true;
            } else {
                lm_lambda *= lm_ni;
                lm_ni *= 2;
                for (int i = tid; i < nv * PSZ; i += NT) pose[i] = pbak[i];   // pop()
                T.sync();
                lm_q++;
                if (rho < 0 && lm_q < 10 && isfinite(lm_lambda)) next_trial = true;
                else { lm_redo = true; }                     // terminate: re-assemble at the restored estimates
            }
        }
        if (done) { lm_left = 0; break; }
        if (lm_redo) { lm_left = 0; continue; }
        if (next_trial) {
            // solve (H + lambda I) x = b with the system of the accepted estimates, then x -> estimates
            bool ok2 = true;
            for (;;) {
                for (int i = tid; i < nv * PSZ; i += NT) pbak[i] = pose[i];   // push()
                if (tid == 0) *T.flag = 0;
                if (use_wave_hw) {
                    // small system: (H + lambda I)^-1 by the register-resident Gauss-Jordan of one wavefront
                    T.sync();
                    if (tid < 64) {
                        double ldt_, tri_;
                        bool okw = wave_spd_inverse(M2, ld, n, tid, lm_lambda, M3, ldt_, tri_);
                        if (!okw && tid == 0) *T.flag = 1;
                    }
                    T.sync();
                } else {
                    for (int i = tid; i < n * ld; i += NT) { int r = i / ld, c = i - r * ld; M3[i] = M2[i] + ((r == c && c < n) ? lm_lambda : 0.0); }
                    T.sync();
                    chol_lower<NT>(T, M3, n, ld);
                }
                ok2 = (*T.flag == 0);
                T.sync();
                if (tid == 0) *T.flag = 0;
                if (ok2) break;
                // the factorisation failed: g2o rejects the step (chi2 = max) without looking at the estimates
                lm_lambda *= lm_ni; lm_ni *= 2; lm_q++;
                if (!(lm_q < 10 && isfinite(lm_lambda))) break;
                T.sync();
            }
            if (!ok2) { lm_redo = true; lm_left = 0; T.sync(); continue; }
            if (use_wave_hw) {
                for (int i = tid; i < n; i += NT) {
                    double sacc = 0;
                    for (int j = 0; j < n; j++) sacc += M3[i * ld + j] * bcur[j];
                    xs[i] = sacc;
                }
                T.sync();
                double sc = 0;
                for (int i = tid; i < n; i += NT) sc += xs[i] * (lm_lambda * xs[i] + bcur[i]);
                sc = T.sum(sc);
                if (tid == 0) xch[2] = sc;
            } else if (tid == 0) {
                for (int i = 0; i < n; i++) {
                    double sacc = bcur[i];
                    for (int kk = 0; kk < i; kk++) sacc -= M3[i * ld + kk] * xs[kk];
                    xs[i] = sacc / M3[i * ld + i];
                }
                for (int i = n - 1; i >= 0; i--) {
                    double sacc = xs[i];
                    for (int kk = i + 1; kk < n; kk++) sacc -= M3[kk * ld + i] * xs[kk];
                    xs[i] = sacc / M3[i * ld + i];
                }
                double sc = 0;
                for (int i = 0; i < n; i++) sc += xs[i] * (lm_lambda * xs[i] + bcur[i]);
                xch[2] = sc;
            }
            T.sync();
            lm_scale = xch[2];
            for (int v = 1 + tid; v < nv; v += NT) {
                const double *dx = xs + (v - 1) * D;
                double *pv = pose + v * PSZ;
                if (D == 6) {
                    // X <- X * fromVectorMQT(dx), renormalised through the quaternion (the estimates are stored as t + q)
                    double Dl[kIso], R[9], q[4];
                    iso_from_mqt(dx, Dl);
#pragma unroll
                    for (int i = 0; i < 3; i++) {
#pragma unroll
                        for (int c = 0; c < 3; c++) R[i * 3 + c] = pv[i * 3] * Dl[c] + pv[i * 3 + 1] * Dl[3 + c] + pv[i * 3 + 2] * Dl[6 + c];
                    }
                    double tn[3];
#pragma unroll
                    for (int i = 0; i < 3; i++) tn[i] = pv[9 + i] + pv[i * 3] * Dl[9] + pv[i * 3 + 1] * Dl[10] + pv[i * 3 + 2] * Dl[11];
                    R_to_quat(R, q);
                    quat_to_R(q, pv);
                    pv[9] = tn[0]; pv[10] = tn[1]; pv[11] = tn[2];
                } else {
                    pv[0] += dx[0]; pv[1] += dx[1]; pv[2] = normalize_theta(pv[2] + dx[2]);
                }
            }
            T.sync();
        }
    }
    }   // LM wrapper
    if (misc[1]) { status = SPG_ST_UNSUPPORTED; finish(); return; }
    // Rows of one n-ary GLC edge in its vertices' update coordinates: Aw = W Jr (rr_ x D q), Jr = the reparametrisation
    // Jacobian at the current estimates (src/glc_edge.cpp:40-49, src/glc_reparam_binary.hpp:78-127). rec = meas (D q) then
    // W (rr_ x D q); vl = the edge's vertices as blanket-local indices; Jq = scratch of q x (Ji0 | Jii), 2 D^2 each.
    auto glc_edge_rows = [&](const double *rec, int q, int rr_, const int *vl, double *Jq, double *Aw) {
        const int dq = D * q;
        for (int i = tid; i < q; i += NT) {
            int v0 = vl[0], vi = vl[i];
            if (D == 6) {
                double Z[kIso], Xz[kIso] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
                iso_from_mqt(rec + 6 * i, Z);
                if (i == 0) se3_edge_jac(Xz, pose + v0 * PSZ, Z, Jq, Jq + DD, nullptr);
                else se3_edge_jac(pose + v0 * PSZ, pose + vi * PSZ, Z, Jq + i * 2 * DD, Jq + i * 2 * DD + DD, nullptr);
            } else {
                double xz[3] = {0, 0, 0};
                if (i == 0) se2_edge_jac(xz, pose + v0 * PSZ, rec, Jq, Jq + DD, nullptr);
                else se2_edge_jac(pose + v0 * PSZ, pose + vi * PSZ, rec + 3 * i, Jq + i * 2 * DD, Jq + i * 2 * DD + DD, nullptr);
            }
        }
        T.sync();
        for (int it = tid; it < rr_ * dq; it += NT) {
            int row = it / dq, col = it - row * dq, blk = col / D, c = col - blk * D;
            const double *Wr = rec + dq + (int64_t)row * dq;
            double sacc = 0;
            if (blk == 0) {
                for (int p = 0; p < D; p++) sacc += Wr[p] * Jq[DD + p * D + c];            // W_0 * J00 (Jj of the mock edge)
                for (int i = 1; i < q; i++)
                    for (int p = 0; p < D; p++) sacc += Wr[i * D + p] * Jq[i * 2 * DD + p * D + c];  // W_i * Ji0
            } else {
                for (int p = 0; p < D; p++) sacc += Wr[blk * D + p] * Jq[blk * 2 * DD + DD + p * D + c];  // W_i * Jii
            }
            Aw[it] = sacc;
        }
        T.sync();
    };
    if constexpr (is_glc) {
        // n-ary GLC edges already in the blanket (a14): H += (W Jr)^T (W Jr)
        double *gA = mat + L.o_gA;
        for (int e = 0; e < bd.n_edge; e++) {
            const spg_edge_ref er = ber[e];
            if (er.kind != SPG_EDGE_GLC) continue;
            const int q = er.nv, dq = D * q, rr_ = (er.len - dq) / dq;
            double *Aw = gA + q * 2 * DD;         // rr_ x dq, behind the Jacobians
            glc_edge_rows(arena + er.off, q, rr_, bev + er.vbegin, gA, Aw);
            for (int it = tid; it < dq * dq; it += NT) {
                int R = it / dq, Cc = it - R * dq;
                double sacc = 0;
                for (int p = 0; p < rr_; p++) sacc += Aw[p * dq + R] * Aw[p * dq + Cc];
                int vR = bev[er.vbegin + R / D], vC = bev[er.vbegin + Cc / D];
                hadd(vR * D + (R % D), vC * D + (Cc % D), sacc);
            }
            T.sync();
        }
    }
    STAMP(1);  // assembled
    const int stop_after = (a.flags >> 8) & 0xff;  // diagnostic: truncate the pipeline (timing breakdowns only)
    if (stop_after == 1) { finish(); return; }

    // ---------------------------------------------------------------- Schur complement (a7)
    if (m == 1) {
        // H_mm is a single d x d block: one lane inverts it in registers (LLT(H_mm).solve, :444-447),
        // then Lambda_t = H_kk - H_mk^T (H_mm^-1 H_mk) as two small products
        if (tid == 0) {
            double Ab[DD], Xr[DD];
#pragma unroll
            for (int i = 0; i < D; i++)
#pragma unroll
                for (int j = 0; j < D; j++) Ab[i * D + j] = Hmm[i * ldm + j];
            if (!chol_reg<D>(Ab)) misc[0] = 1;
            chol_inverse_reg<D>(Ab, Xr);
#pragma unroll
            for (int i = 0; i < D; i++)
#pragma unroll
                for (int j = 0; j < D; j++) Hmm[i * ldm + j] = Xr[i * D + j];
        }
        T.sync();
        STAMP(26);  // Hmm inverse
        if (misc[0]) { status = SPG_ST_HMM_NOT_PD; finish(); return; }
        // Y = H_mm^-1 H_mk into M2 rows 0..D-1 (M2 is free until Chow-Liu)
        for (int it = tid; it < D * n; it += NT) {
            int r = it / n, c = it - r * n;
            double s = 0;
#pragma unroll
            for (int p = 0; p < D; p++) s += Hmm[r * ldm + p] * Hmk[p * ld + c];
            M2[r * ld + c] = s;
        }
        T.sync();
        STAMP(27);  // Y
    } else {
        chol_lower<NT>(T, Hmm, nm, ldm);
        if (misc[0]) { status = SPG_ST_HMM_NOT_PD; finish(); return; }
        tri_solve_lower<NT>(T, Hmm, nm, ldm, Hmk, n, ld);
    }
    {
        int sh = ceil_log2(n), tot = n << sh;
        double bad = 0;
        const double *Yl = (m == 1) ? M2 : Hmk;   // m == 1: Hmk^T (Hmm^-1 Hmk) ; else (L^-1 Hmk)^T (L^-1 Hmk)
        for (int it = tid; it < tot; it += NT) {
            int i = it >> sh, j = it & ((1 << sh) - 1);
            if (j < n) {
                double s = 0;
                if (m == 1) {
#pragma unroll
                    for (int p = 0; p < D; p++) s += Hmk[p * ld + i] * Yl[p * ld + j];
                } else {
                    for (int p = 0; p < nm; p++) s += Hmk[p * ld + i] * Yl[p * ld + j];
                }
                double v = M1[i * ld + j] - s;
                M1[i * ld + j] = v;
                if (!isfinite(v)) bad = 1;
            }
        }
        double anybad = T.sum(bad);
        STAMP(28);  // Lambda update
        mirror_upper<NT>(T, M1, n, ld);
        if (anybad > 0) { status = SPG_ST_NONFINITE; finish(); return; }
    }
    if (bd.tinfo_off >= 0 && !stamping) {
        double *dst = arena + bd.tinfo_off;
        for (int it = tid; it < n * n; it += NT) { int i = it / n, j = it - i * n; dst[it] = M1[i * ld + j]; }
    }
    // pseudo-Chow-Liu tree of the kept vertices (a8): fills pairs[0..2(k-1)) in pop order, sets min_gap
    auto chow_liu_tree = [&](const auto TT) -> int {
        if (k == 2) {
            if (TT.tid == 0) { pairs[0] = 0; pairs[1] = 1; }
            TT.sync();
            return (int)SPG_OK;
        }
        // Sigma~ = (Lambda_t + 1 I)^-1 in M2
        if ((use_wave_hw && TT.size == 64)) {
            double ld_, tr_;
            bool ok_ = wave_spd_inverse(M1, ld, n, TT.tid, 1.0, M2, ld_, tr_);
            if (!ok_) return (int)SPG_ST_TIKHONOV_NOT_PD;
            TT.sync();
        } else {
            for (int it = TT.tid; it < n * ld; it += TT.size) M2[it] = M1[it];
            TT.sync();
            for (int i = TT.tid; i < n; i += TT.size) M2[i * ld + i] += 1.0;
            TT.sync();
            chol_lower(TT, M2, n, ld, ev);
            if ((*TT.flag)) return (int)SPG_ST_TIKHONOV_NOT_PD;
            CSTAMP(3);  // cl chol
            tri_inverse_lower(TT, M2, M3, n, ld, ev);
            CSTAMP(4);  // cl triinv
            gram_lower_inverse(TT, M3, M2, n, ld);
        }
        CSTAMP(5);  // cl gram
        // per-vertex diagonal blocks: Cholesky + log det
        for (int v = TT.tid; v < k; v += TT.size) {
            double Ab[DD];
#pragma unroll
            for (int r = 0; r < D; r++)
#pragma unroll
                for (int c = 0; c < D; c++) Ab[r * D + c] = M2[(v * D + r) * ld + v * D + c];
            if (!chol_reg<D>(Ab)) (*TT.flag) = 1;
            LogProd lp;
#pragma unroll
            for (int r = 0; r < D; r++) {
                lp.mul(Ab[r * D + r]);
                // keep 1/L_rr on the diagonal of the staged factor: the pair solves below multiply by it
#pragma unroll
                for (int c = 0; c < D; c++) Lb[v * DD + r * D + c] = (r == c) ? fast_rcp(Ab[r * D + r]) : Ab[r * D + c];
            }
            ldb[v] = 2.0 * lp.value();
        }
        TT.sync();
        CSTAMP(6);  // cl vertex chol
        // pair weights w = ld_i + ld_j - ld_{ij}, ld_{ij} = ld_i + logdet(S_jj - S_ji S_ii^-1 S_ij)
        for (int p = TT.tid; p < L.P; p += TT.size) {
            int i = 0, rem = p;
            while (rem >= k - 1 - i) { rem -= k - 1 - i; i++; }
            int j = i + 1 + rem;
            pij[2 * p] = i; pij[2 * p + 1] = j;
            const double *Li = Lb + i * DD;
            double Y[DD];
#pragma unroll
            for (int c = 0; c < D; c++) {
#pragma unroll
                for (int r = 0; r < D; r++) {
                    double s = M2[(i * D + r) * ld + j * D + c];
#pragma unroll
                    for (int q = 0; q < D; q++) if (q < r) s -= Li[r * D + q] * Y[q * D + c];
                    Y[r * D + c] = s * Li[r * D + r];  // diagonal holds the reciprocal
                }
            }
            double Sb[DD];
#pragma unroll
            for (int r = 0; r < D; r++)
#pragma unroll
                for (int c = 0; c < D; c++) if (c <= r) {
                    double s = M2[(j * D + r) * ld + j * D + c];
#pragma unroll
                    for (int q = 0; q < D; q++) s -= Y[q * D + r] * Y[q * D + c];
                    Sb[r * D + c] = s;
                }
            if (!chol_reg<D>(Sb)) (*TT.flag) = 1;
            LogProd lp;
#pragma unroll
            for (int r = 0; r < D; r++) lp.mul(Sb[r * D + r]);
            double lxy = ldb[i] + 2.0 * lp.value();
            w[p] = -((ldb[i] + ldb[j]) - lxy);  // stored negated: ascending sort == max-heap pop order
        }
        TT.sync();
        if ((*TT.flag)) return (int)SPG_ST_TIKHONOV_NOT_PD;
        CSTAMP(7);  // cl pair weights
        sort_ascending(TT, w, 1, L.P, sorted);
        CSTAMP(8);  // cl sort
        if (TT.tid == 0) {
            // Kruskal in pop order (src/pseudo_chow_liu.cpp:253-289); first `ne` of the bin are used
            for (int v = 0; v < k; v++) comp[v] = v;
            int nacc = 0, last = 0;
            // accepted edges first; rejected ones are only needed when ne > k-1, which has no closed form
            for (int s = 0; s < L.P && nacc < k - 1; s++) {
                int p = sorted[s];
                int i = pij[2 * p], j = pij[2 * p + 1];
                int ci = comp[i], cj = comp[j];
                if (ci != cj) {
                    pairs[2 * nacc] = i; pairs[2 * nacc + 1] = j;
                    nacc++;
                    for (int v = 0; v < k; v++) if (comp[v] == cj) comp[v] = ci;
                }
                last = s;
            }
            int upto = min(last + 1, L.P - 1);
            double g = __builtin_inf();
            for (int s = 0; s < upto; s++) {
                double x = -w[sorted[s]], y = -w[sorted[s + 1]];
                double den = fmax(fmax(fabs(x), fabs(y)), 1e-300);
                g = fmin(g, (x - y) * fast_rcp(den));
            }
            cs[0] = g;
        }
        TT.sync();
        min_gap = cs[0];
        TT.sync();
        CSTAMP(29);  // cl kruskal + gap done
        return (int)SPG_OK;
    };
    if constexpr (is_glc) {
#include "spg_glc_tail.inc"
    }
    STAMP(2);  // schur
    if (k < 2 || stop_after == 2) { finish(); return; }

    // ---------------------------------------------------------------- sparsity pattern (a8)
    int ne;
    {
        int msub = (int)((1 + a.chord_ratio) * (k - 1));
        bool full = msub >= k * (k - 1) / 2;
        if (k == 2) ne = 1;
        else if (a.topology == SPG_TOPO_TREE) ne = k - 1;
        else if (a.topology == SPG_TOPO_DENSE || (a.topology == SPG_TOPO_SUBGRAPH && full)) ne = k * (k - 1) / 2;
        else if (a.topology == SPG_TOPO_SUBGRAPH) ne = msub;
        else { status = SPG_ST_UNSUPPORTED; finish(); return; }
        if (ne * D != n - D) {
            // Chow-Liu still runs in the reference before optimizeInformation discovers that no closed
            // form exists (src/optimizer.cpp:21); the interior-point branch is out of scope.
            status = SPG_ST_NEEDS_INTERIOR_POINT; finish(); return;
        }
    }

    // ================================================================ information recovery (a11, a12)
    // Two routes to the same numbers.
    //  * eigen route — the reference's own: eig(Lambda_t), drop the d gauge directions, Sigma = U S U^T
    //    (src/logdet_function.cpp:14-64,236-279), KLD through M = U^T A U (src/logdet_function.cpp:119-133).
    //  * gauge route — Lambda_t of a blanket of relative-pose edges has an exactly known d-dimensional
    //    null space: the rigid motions of the whole blanket, N = [G_1; ...; G_k] in the vertices' update
    //    coordinates. With N^ an orthonormal basis of it and C = Lambda_t + N^ N^^T (SPD):
    //        U S U^T = C^-1 - N^ N^^T,   J_e N^ = 0  =>  J_e Sigma J_e^T = J_e C^-1 J_e^T,
    //        log det S = -log det C,  tr(S M) = tr(C^-1 A),  log det(U^T A U) = log det(A + N^ N^^T),
    //    so three Cholesky factorisations replace the Jacobi eigen-decomposition (~10x fewer dependent
    //    steps). It is taken only when ||C^-1||_F < 5e4, which proves lambda_{d+1}(Lambda_t) > 1e-5, i.e.
    //    the reference's `smalleigs <= dim` branch; anything else (rank-deficient blankets, failed
    //    factorisations) goes through the eigen route. tests/test_gpu_parity.py checks both routes
    //    against the oracle to 1e-9.
    const int r = n - D;
    double *Ng = smem + L.o_Ng;      // n x D orthonormal gauge basis
    double *tre = smem + L.o_tre;    // per-edge tr(X_e B_e)
    bool gauge_ok = false;
    double logdetS = 0.0;
    double *Sg = M1, *Scr = M3;      // Sigma and scratch for the closed form (swapped on the gauge route)
    auto gauge_chain = [&](const auto TT) {
        gauge_basis_raw<D>(TT, pose + m * PSZ, k, Ng);
        CSTAMP(11);  // gauge basis
        gauge_orthonormalise<D>(TT, n, Ng, eT);
        CSTAMP(12);  // orthonormalised
        // ---- C = Lambda_t + N^ N^^T into M3, Cholesky, inverse
        gauge_regularised<D>(TT, M1, ld, n, Ng, M3);
        CSTAMP(13);  // C formed
        if ((use_wave_hw && TT.size == 64)) {
            double ldC, trC;
            bool ok_ = wave_spd_inverse(M3, ld, n, TT.tid, 0.0, M3, ldC, trC);
            bool fail = !ok_ || ((*TT.flag) != 0);
            TT.sync();
            if (TT.tid == 0) { (*TT.flag) = 0; }
            TT.sync();
            // trace(C^-1) >= lambda_max(C^-1): below 5e4 proves lambda_{d+1}(Lambda_t) > 1e-5
            if (!fail && trC < 5e4 && isfinite(trC)) {
                if (TT.tid == 0) { xch[0] = 1.0; xch[1] = -ldC; }
            }
            CSTAMP(30);  // gauge inverse done
        } else {
            chol_lower(TT, M3, n, ld, Sv);
            CSTAMP(14);  // C chol
            bool fail = ((*TT.flag) != 0);
            TT.sync();
            if (TT.tid == 0) { (*TT.flag) = 0; }
            TT.sync();
            if (!fail) {
                double ldC = chol_logdet(TT, M3, n, ld);
                CSTAMP(15);  // logdet
                tri_inverse_lower(TT, M3, M2, n, ld, Sv);
                CSTAMP(16);  // triinv
                // C^-1 = Li^T Li into M3 with its Frobenius norm
                int sh = ceil_log2(n), tot = n << sh;
                double f2 = 0;
                for (int it = TT.tid; it < tot; it += TT.size) {
                    int i = it >> sh, j = it & ((1 << sh) - 1);
                    if (j <= i) {
                        double s = 0;
                        for (int q = i; q < n; q++) s += M2[q * ld + i] * M2[q * ld + j];
                        M3[i * ld + j] = s;
                        M3[j * ld + i] = s;
                        f2 += (i == j) ? s * s : 2.0 * s * s;
                    }
                }
                double fro2 = TT.sum(f2);
                if (fro2 < 5e4 * 5e4 && isfinite(fro2)) {
                    if (TT.tid == 0) { xch[0] = 1.0; xch[1] = -ldC; }
                }
            }
        }
    };
    // ---- run the two independent chains: Chow-Liu (Lambda_t + I)^-1 ... Kruskal, and the gauge route's
    // C^-1. With two wavefronts per blanket (NT == 128) they run side by side, each wavefront as its own
    // team with wave-local barriers; otherwise one after the other on the whole team.
    if (tid == 0) { xch[0] = 0.0; xch[1] = 0.0; }
    T.sync();
    {
        int st_ = SPG_OK;
        if (split) {
            Team<64> S{tid & 63, nullptr, misc + ((tid < 64) ? 6 : 2)};
            if (tid < 64) { int s2 = chow_liu_tree(S); if (S.tid == 0) misc[7] = s2; }
            else gauge_chain(S);
            T.sync();
            st_ = misc[7];
            min_gap = (k > 2) ? cs[0] : min_gap;
        } else {
            st_ = chow_liu_tree(T);
            if (st_ == SPG_OK && !(a.flags & SPG_FLAG_FORCE_EIG)) gauge_chain(T);
        }
        if (st_ != SPG_OK) { status = st_; finish(); return; }
        T.sync();
        if (xch[0] != 0.0) { gauge_ok = true; logdetS = xch[1]; Sg = M3; Scr = M1; }
        T.sync();
        if (tid == 0) { misc[0] = 0; misc[2] = 0; misc[6] = 0; }
        T.sync();
    }
    STAMP(9);  // both chains done
    if (stop_after == 3) { finish(); return; }
    // ---------------------------------------------------------------- new edge skeleton (a9, a10)
    for (int e = tid; e < ne; e += NT) {
        int va = m + pairs[2 * e], vb = m + pairs[2 * e + 1];
        double *rec = arena + bd.new_off + (int64_t)e * REC;
        if (D == 6) {
            double Z[kIso], q[4];
            iso_inv_mul(pose + va * PSZ, pose + vb * PSZ, Z);
            R_to_quat(Z, q);
            double *rw = COH ? (recbuf + e * REC) : rec;
            rw[0] = Z[9]; rw[1] = Z[10]; rw[2] = Z[11]; rw[3] = q[0]; rw[4] = q[1]; rw[5] = q[2]; rw[6] = q[3];
            se3_edge_jac(pose + va * PSZ, pose + vb * PSZ, Z, nJ + e * 2 * DD, nJ + e * 2 * DD + DD, nullptr);
        } else {
            double z[3];
            se2_between(pose + va * PSZ, pose + vb * PSZ, z);
            double *rw = COH ? (recbuf + e * REC) : rec;
            rw[0] = z[0]; rw[1] = z[1]; rw[2] = z[2];
            se2_edge_jac(pose + va * PSZ, pose + vb * PSZ, z, nJ + e * 2 * DD, nJ + e * 2 * DD + DD, nullptr);
        }
    }
    T.sync();
    if (ne == 1) {
        // single-measurement case goes through sparseJacobian(): entries below epsilon are dropped
        // (src/logdet_function.cpp:243-247,335)
        for (int it = tid; it < 2 * DD; it += NT) if (fabs(nJ[it]) < 2.220446049250313e-16) nJ[it] = 0.0;
        T.sync();
    }

    STAMP(10);  // new edges
    if (stop_after == 4) { finish(); return; }
    if (!gauge_ok) {
        // ------------------------------------------------------------ eigen route: spectrum of Lambda_t
        for (int it = tid; it < n * ld; it += NT) M3[it] = M1[it];
        T.sync();
        if (!jacobi_eigh<NT>(T, M3, M2, n, ld, cs)) { status = SPG_ST_EIG_FAIL; finish(); return; }
        for (int i = tid; i < n; i += NT) ev[i] = M3[i * ld + i];
        T.sync();
        if (stop_after == 5) { finish(); return; }
        sort_ascending<NT>(T, ev, 1, n, perm);
        {
            double cnt = 0;
            for (int i = tid; i < n; i += NT) cnt += (ev[i] < 1e-5) ? 1.0 : 0.0;
            int smalleigs = (int)T.sum(cnt);
            if (smalleigs <= D) {
                for (int j = tid; j < r; j += NT) { int idx = perm[D + j]; keep[j] = idx; Sv[j] = 1.0 / ev[idx]; }
            } else {
                info |= SPG_INFO_RANK_DEFICIENT;
                if (tid == 0) {
                    // chooseDimensions (src/logdet_function.cpp:66-81): drop the D candidates with the
                    // smallest ||J u||; S clamped as at src/logdet_function.cpp:55
                    double *nrm = cs;  // smalleigs <= n doubles
                    for (int c = 0; c < smalleigs; c++) {
                        int col = perm[c];
                        double s2 = 0;
                        for (int e = 0; e < ne; e++) {
                            int oa = pairs[2 * e] * D, ob = pairs[2 * e + 1] * D;
                            const double *Ja = nJ + e * 2 * DD, *Jb = Ja + DD;
                            for (int rr = 0; rr < D; rr++) {
                                double s = 0;
                                for (int p = 0; p < D; p++) {
                                    double ja = Ja[rr * D + p], jb = Jb[rr * D + p];
                                    if (fabs(ja) >= 2.220446049250313e-16) s += ja * M2[(oa + p) * ld + col];
                                    if (fabs(jb) >= 2.220446049250313e-16) s += jb * M2[(ob + p) * ld + col];
                                }
                                s2 += s * s;
                            }
                        }
                        nrm[c] = sqrt(s2);
                    }
                    // mark the D smallest (norm, then sorted position); keep[] doubles as the mark array
                    for (int i = 0; i < n; i++) keep[i] = 0;
                    for (int t = 0; t < D; t++) {
                        int best = -1;
                        for (int c = 0; c < smalleigs; c++) {
                            if (keep[c]) continue;
                            if (best < 0 || nrm[c] < nrm[best]) best = c;
                        }
                        keep[best] = 1;
                    }
                    double lmax = ev[perm[n - 1]];
                    int j = 0;
                    // compact in place: positions are visited in ascending order and j <= i always
                    for (int i = 0; i < n; i++) {
                        bool dropped = keep[i] != 0;
                        if (!dropped) {
                            int idx = perm[i];
                            keep[j] = idx;
                            Sv[j] = fmin(fabs(1.0 / ev[idx]), 1e6 / lmax);
                            j++;
                        }
                    }
                }
            }
            T.sync();
        }
        {
            double s = 0;
            for (int j = tid; j < r; j += NT) s += log(Sv[j]);
            logdetS = T.sum(s);
        }
        // Sigma = U S U^T into M1
        {
            int sh = ceil_log2(n), tot = n << sh;
            for (int it = tid; it < tot; it += NT) {
                int i = it >> sh, j = it & ((1 << sh) - 1);
                if (j <= i) {
                    double s = 0;
                    for (int q = 0; q < r; q++) { int c = keep[q]; s += M2[i * ld + c] * Sv[q] * M2[j * ld + c]; }
                    M1[i * ld + j] = s;
                    M1[j * ld + i] = s;
                }
            }
            T.sync();
        }
    }
    STAMP(17);  // Cinv+guard
    if (stop_after == 6) { finish(); return; }

    // ---------------------------------------------------------------- closed form X_e (a11)
    {
        double *Pw = Scr;               // ne x 3 x DD
        double *Bk = Scr + ne * 3 * DD; // ne x DD
        for (int it = tid; it < ne * 3 * DD; it += NT) {
            int e = it / (3 * DD), rem = it - e * 3 * DD, wch = rem / DD, rc = rem - wch * DD, rr = rc / D, c = rc - rr * D;
            int oa = pairs[2 * e] * D, ob = pairs[2 * e + 1] * D;
            const double *J = nJ + e * 2 * DD + (wch == 2 ? DD : 0);
            int ro = (wch == 2) ? ob : oa, co = (wch == 0) ? oa : ob;
            double s = 0;
#pragma unroll
            for (int p = 0; p < D; p++) s += J[rr * D + p] * Sg[(ro + p) * ld + co + c];
            Pw[it] = s;
        }
        T.sync();
        STAMP(31);  // closed form: J Sigma
        for (int it = tid; it < ne * DD; it += NT) {
            int e = it / DD, rc = it - e * DD, rr = rc / D, c = rc - rr * D;
            const double *Ja = nJ + e * 2 * DD, *Jb = Ja + DD;
            const double *P0 = Pw + e * 3 * DD, *P1 = P0 + DD, *P2 = P1 + DD;
            double t1rc = 0, t1cr = 0, t2rc = 0, t2cr = 0, t3rc = 0, t3cr = 0;
#pragma unroll
            for (int p = 0; p < D; p++) {
                t1rc += P0[rr * D + p] * Ja[c * D + p]; t1cr += P0[c * D + p] * Ja[rr * D + p];
                t2rc += P1[rr * D + p] * Jb[c * D + p]; t2cr += P1[c * D + p] * Jb[rr * D + p];
                t3rc += P2[rr * D + p] * Jb[c * D + p]; t3cr += P2[c * D + p] * Jb[rr * D + p];
            }
            double v = (ne == 1) ? (t1rc + t2rc + t2cr + t3rc)
                                 : (0.5 * (t1rc + t1cr) + (t2rc + t2cr) + 0.5 * (t3rc + t3cr));
            Bk[it] = v;
        }
        T.sync();
        STAMP(32);  // closed form: B_e
        for (int e = tid; e < ne; e += NT) {
            double Ab[DD], Xr[DD];
#pragma unroll
            for (int i = 0; i < DD; i++) Ab[i] = Bk[e * DD + i];
            double trs = 0;
            if (!chol_reg<D>(Ab)) misc[0] = 1;
            chol_inverse_reg<D>(Ab, Xr);
            double *rec = COH ? (recbuf + e * REC + PS) : (arena + bd.new_off + (int64_t)e * REC + PS);
            int pidx = 0;
#pragma unroll
            for (int i = 0; i < D; i++)
#pragma unroll
                for (int j = 0; j < D; j++) {
                    X[e * DD + i * D + j] = Xr[i * D + j];
                    trs += Xr[i * D + j] * Bk[e * DD + ((j <= i) ? (i * D + j) : (j * D + i))];
                    if (j >= i) rec[pidx++] = Xr[i * D + j];
                }
            tre[e] = trs;
        }
        T.sync();
        STAMP(33);  // closed form: X_e = B_e^-1, records written
        if (misc[0]) { status = SPG_ST_CLOSED_FORM_NOT_PD; finish(); return; }
    }
    n_new = ne;
    publish();  // the graph update can proceed; the KLD below is reported later
    STAMP(18);  // closed form
    if (stop_after == 7) { finish(); return; }

    // ---------------------------------------------------------------- per-blanket KLD (a12)
    {
        // A = J^T X J (upper blocks accumulated, then mirrored) into Am
        double *Am = gauge_ok ? M2 : M1;
        double *XJ = gauge_ok ? M1 : M3;  // ne x 2 x DD
        for (int it = tid; it < ne * 2 * DD; it += NT) {
            int e = it / (2 * DD), rem = it - e * 2 * DD, wch = rem / DD, rc = rem - wch * DD, rr = rc / D, c = rc - rr * D;
            const double *J = nJ + e * 2 * DD + wch * DD;
            double s = 0;
#pragma unroll
            for (int p = 0; p < D; p++) s += X[e * DD + rr * D + p] * J[p * D + c];
            XJ[it] = s;
        }
        for (int it = tid; it < n * ld; it += NT) Am[it] = 0.0;
        T.sync();
        for (int e = 0; e < ne; e++) {
            int oa = pairs[2 * e] * D, ob = pairs[2 * e + 1] * D;
            const double *Ja = nJ + e * 2 * DD, *Jb = Ja + DD;
            const double *XJa = XJ + e * 2 * DD, *XJb = XJa + DD;
            for (int it = tid; it < 3 * DD; it += NT) {
                int blk = it / DD, rc = it - blk * DD, rr = rc / D, c = rc - rr * D;
                const double *Jl = (blk == 2) ? Jb : Ja;
                const double *Xr_ = (blk == 0) ? XJa : XJb;
                double s = 0;
#pragma unroll
                for (int p = 0; p < D; p++) s += Jl[p * D + rr] * Xr_[p * D + c];
                int R = ((blk == 2) ? ob : oa) + rr, Cc = ((blk == 0) ? oa : ob) + c;
                Am[R * ld + Cc] += s;
            }
            T.sync();
        }
        mirror_upper<NT>(T, Am, n, ld);
        STAMP(19);  // A assembled
        if (gauge_ok) {
            // kld = 1/2 ( tr(C^-1 A) - log det(A + N^ N^^T) + log det C - r ), tr(C^-1 A) = sum_e tr(X_e B_e)
            gauge_add<D>(T, Am, ld, n, Ng);
            double tr;
            {
                double s = 0;
                for (int e = tid; e < ne; e += NT) s += tre[e];
                tr = T.sum(s);
            }
            STAMP(20);  // A + NN
            if (use_wave_hw && NT <= 128) {
                // the first wavefront factorises in registers; the result reaches every lane through LDS
                if (tid < 64) {
                    double ldA_;
                    bool ok_ = wave_spd_logdet(Am, ld, n, tid, ldA_);
                    if (tid == 0) { xch[2] = ok_ ? 1.0 : 0.0; xch[3] = ldA_; }
                }
                T.sync();
                if (xch[2] == 0.0) { kld = __builtin_inf(); status = SPG_ST_KLD_NOT_PD; }
                else kld = 0.5 * (tr - xch[3] - logdetS - (double)r);
            } else {
                chol_lower<NT>(T, Am, n, ld);
                if (misc[0]) {
                    kld = __builtin_inf();
                    status = SPG_ST_KLD_NOT_PD;
                } else {
                    double ldA = chol_logdet<NT>(T, Am, n, ld);
                    kld = 0.5 * (tr - ldA - logdetS - (double)r);
                }
            }
            STAMP(21);  // chol A
        } else {
            // Tm = A * U_kept  (n x r) into M3 ; XJ no longer needed
            int shr = ceil_log2(r > 0 ? r : 1);
            for (int it = tid; it < (n << shr); it += NT) {
                int i = it >> shr, j = it & ((1 << shr) - 1);
                if (j < r) {
                    int c = keep[j];
                    double s = 0;
                    for (int p = 0; p < n; p++) s += M1[i * ld + p] * M2[p * ld + c];
                    M3[i * ld + j] = s;
                }
            }
            T.sync();
            // M = U_kept^T Tm  (r x r) into M1 (upper needed, lower mirrored)
            for (int it = tid; it < (r << shr); it += NT) {
                int i = it >> shr, j = it & ((1 << shr) - 1);
                if (j < r && j >= i) {
                    int c = keep[i];
                    double s = 0;
                    for (int p = 0; p < n; p++) s += M2[p * ld + c] * M3[p * ld + j];
                    M1[i * ld + j] = s;
                    M1[j * ld + i] = s;
                }
            }
            T.sync();
            double tr;
            {
                double s = 0;
                for (int i = tid; i < r; i += NT) s += M1[i * ld + i] * Sv[i];
                tr = T.sum(s);
            }
            chol_lower<NT>(T, M1, r, ld);
            if (misc[0]) {
                kld = __builtin_inf();
                status = SPG_ST_KLD_NOT_PD;
            } else {
                double ldM = chol_logdet<NT>(T, M1, r, ld);
                kld = 0.5 * (tr - ldM - logdetS - (double)r);
            }
        }
    }
    STAMP(22);  // end
    finish();
}

template <int D, int NT, bool GWS, int ALG>
__global__ void __launch_bounds__(NT) blanket_kernel(KArgs a) {
    extern __shared__ double smem[];
    const int b = a.list[blockIdx.x];
    const spg_blanket_desc bd = a.blk[b];
    blanket_body<D, NT, GWS, ALG>(a, bd, a.vpo + bd.vert_begin, a.er + bd.edge_begin, a.ev, (int)blockIdx.x, smem);
}

// ---------------------------------------------------------------------------------- Local linearisation point, pre-pass
// buildSubgraph with SparsityOptions::Local (src/vertex_remover.cpp:304-391) for the blankets the generic NFR kernel takes
// (interior point, correlated patterns, clusters): the blanket's estimates are copied into a scratch block; if every vertex
// but the first removed one sits in exactly one pose-pose edge they are re-initialised in closed form (the first removed
// vertex at the origin, each neighbour at z or z^-1 of its edge, edges in blanket order: :304-381) and flag = 1; otherwise
// flag = 0 and the host runs the 10 LM iterations with that vertex fixed (:382-391) on the scratch block. The kernels that
// follow read the blanket's poses from the scratch block (their pose offsets are redirected) and take them as they are.
__device__ __forceinline__ void tq_rotate(const double *q, const double *v, double *o) {
    const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
    const double cx = uy * v[2] - uz * v[1], cy = uz * v[0] - ux * v[2], cz = ux * v[1] - uy * v[0];
    o[0] = v[0] + 2.0 * (w * cx + (uy * cz - uz * cy));
    o[1] = v[1] + 2.0 * (w * cy + (uz * cx - ux * cz));
    o[2] = v[2] + 2.0 * (w * cz + (ux * cy - uy * cx));
}
__device__ __forceinline__ void tq_compose(const double *a, const double *b, double *o) {   // o = a * b (may alias neither)
    double r[3];
    tq_rotate(a + 3, b, r);
    o[0] = a[0] + r[0]; o[1] = a[1] + r[1]; o[2] = a[2] + r[2];
    const double ax = a[3], ay = a[4], az = a[5], aw = a[6], bx = b[3], by = b[4], bz = b[5], bw = b[6];
    double x = aw * bx + ax * bw + ay * bz - az * by, y = aw * by - ax * bz + ay * bw + az * bx,
           z = aw * bz + ax * by - ay * bx + az * bw, w = aw * bw - ax * bx - ay * by - az * bz;
    const double nn = 1.0 / sqrt(x * x + y * y + z * z + w * w), sg = (w < 0) ? -nn : nn;
    o[3] = x * sg; o[4] = y * sg; o[5] = z * sg; o[6] = w * sg;
}
__device__ __forceinline__ void tq_inverse(const double *a, double *o) {
    double q[4] = {-a[3], -a[4], -a[5], a[6]}, r[3];
    tq_rotate(q, a, r);
    o[0] = -r[0]; o[1] = -r[1]; o[2] = -r[2]; o[3] = q[0]; o[4] = q[1]; o[5] = q[2]; o[6] = q[3];
}

template <int D>
__global__ __launch_bounds__(64) void local_point_kernel(const double *arena, double *lpose, const spg_blanket_desc *blk, const int64_t *vpo,
                                                         const spg_edge_ref *er, const int32_t *ev, const int32_t *list, const int64_t *lp_off, int32_t *flag) {
    constexpr int PS = (D == 6) ? 7 : 3;
    __shared__ int cnt[1024];
    const int tid = threadIdx.x;
    const spg_blanket_desc bd = blk[list[blockIdx.x]];
    const int nv = bd.n_vert;
    double *P = lpose + lp_off[blockIdx.x];
    for (int it = tid; it < nv * PS; it += 64) P[it] = arena[vpo[bd.vert_begin + it / PS] + it % PS];
    for (int v = tid; v < nv && v < 1024; v += 64) cnt[v] = 0;
    __syncthreads();
    if (tid != 0) return;
    bool ok = nv <= 1024;
    for (int e = 0; ok && e < bd.n_edge; e++) {
        const spg_edge_ref r = er[bd.edge_begin + e];
        if (r.kind != SPG_EDGE_BINARY) { ok = false; break; }
        const int vi = ev[r.vbegin], vj = ev[r.vbegin + 1];
        if (vi != 0) cnt[vi]++;
        if (vj != 0) cnt[vj]++;
    }
    for (int v = 1; ok && v < nv; v++) if (cnt[v] > 1) ok = false;
    if (ok) {
        if (D == 3) { P[0] = 0; P[1] = 0; P[2] = 0; }
        else { P[0] = 0; P[1] = 0; P[2] = 0; P[3] = 0; P[4] = 0; P[5] = 0; P[6] = 1; }
        for (int e = 0; e < bd.n_edge; e++) {
            const spg_edge_ref r = er[bd.edge_begin + e];
            const int vi = ev[r.vbegin], vj = ev[r.vbegin + 1];
            if (vi == 0 && vj == 0) continue;
            const double *z = arena + r.off;
            if (D == 3) {
                if (vi == 0) {
                    const double c = cos(P[2]), sn = sin(P[2]);
                    double *o = P + vj * 3;
                    o[0] = P[0] + c * z[0] - sn * z[1]; o[1] = P[1] + sn * z[0] + c * z[1]; o[2] = normalize_theta(P[2] + z[2]);
                } else {
                    const double cz = cos(z[2]), sz = sin(z[2]);
                    const double zi[3] = {-(cz * z[0] + sz * z[1]), -(-sz * z[0] + cz * z[1]), normalize_theta(-z[2])};
                    const double *a = P + vj * 3;
                    const double c = cos(a[2]), sn = sin(a[2]);
                    const double ox = a[0] + c * zi[0] - sn * zi[1], oy = a[1] + sn * zi[0] + c * zi[1], ot = normalize_theta(a[2] + zi[2]);
                    double *o = P + vi * 3;
                    o[0] = ox; o[1] = oy; o[2] = ot;
                }
            } else {
                double zq[7], out[7];
                for (int i = 0; i < 7; i++) zq[i] = z[i];
                { const double nn = 1.0 / sqrt(zq[3] * zq[3] + zq[4] * zq[4] + zq[5] * zq[5] + zq[6] * zq[6]); for (int i = 3; i < 7; i++) zq[i] *= nn; }
                if (vi == 0) { tq_compose(P, zq, out); for (int i = 0; i < 7; i++) P[vj * 7 + i] = out[i]; }
                else { double zi[7]; tq_inverse(zq, zi); tq_compose(P + vj * 7, zi, out); for (int i = 0; i < 7; i++) P[vi * 7 + i] = out[i]; }
            }
        }
    }
    flag[blockIdx.x] = ok ? 1 : 0;
}

// ---------------------------------------------------------------------------------- persistent worker
// Narrow rounds (a few dozen blankets that depend on the previous few dozen) are bound by the launch-to-result latency
// of a batch, not by arithmetic. For them the device runs ONE long-lived kernel per marginalisation: kWorkerWGs
// workgroups that take tickets from a queue in fine-grained device memory which the host fills through the PCIe BAR
// (posted stores: blanket packets, then the item slots, then `tail`). A batch then costs the host a few cache-line
// writes instead of a kernel launch, and reaches a workgroup ~1-2 us after the store of `tail` instead of ~15 us after
// hipLaunchKernel. Results travel as before (out records in the pinned host mailbox, ready / final words).
//
// Packet of one blanket (8-byte words; written by the host, read with system-scope loads):
//   [0] arena  [1] mailbox (device address, 0 = none)  [2] mail_base  [3] out_off  [4] new_off  [5] tinfo_off
//   [6] n_vert | n_remove << 32   [7] n_edge | n_new_max << 32   [8] n_new_vert_max | scratch << 32
//   [9] topology | flags << 32    [10] lin_point | tag << 32     [11] chord_ratio (f64 bits)
//   [12] n_words | 0              then vpo[n_vert] (i64), er[n_edge] (spg_edge_ref, 3 words each, vbegin relative to the
//   packet's ev), ev (i32 pairs)
using spg::kQCap; using spg::kPktHdr; using spg::kPktWords; using spg::kPktStride; using spg::kWorkerMaxN; using spg::kBells; using spg::kBellStride;
using spg::WorkQ;

__device__ __forceinline__ unsigned long long load_sys(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}


template <int D, int ALG>
__global__ void __launch_bounds__(128) blanket_worker(WorkQ *q, unsigned long long *ticket, long long idle_ticks, int n_bells, int lazy) {
    extern __shared__ double smem[];
    __shared__ unsigned long long pk[kPktWords];
    __shared__ unsigned long long s_item;
    const int tid = threadIdx.x;
    for (;;) {
        if (tid == 0) {
            const unsigned long long my = atomicAdd(ticket, 1ULL);
            unsigned long long it = 0;
            long long t0 = wall_clock64();
            unsigned long long seen = ~0ULL;
            for (;;) {
                // (relaxed: an acquire here would invalidate this XCD's L1 / L2 on every poll of every idle workgroup — the item and
                //  the packet are read with system-scope loads that bypass the caches anyway)
                const unsigned long long tail = load_sys(&q->tail[(blockIdx.x % n_bells) * kBellStride]);
                if (tail > my) { it = load_sys(&q->item[my % kQCap]); break; }
                if (load_sys(&q->stop)) break;
                if (tail != seen) { seen = tail; t0 = wall_clock64(); }
                else if (wall_clock64() - t0 > idle_ticks) break;   // the host went away: every wave must be able to leave
                // the next few tickets poll back to back, the others doze (one poll is an uncached HBM read)
                const unsigned long long ahead = my - tail;
                if (lazy) {
                    if (ahead >= 2) for (int z = 0; z < lazy; z++) __builtin_amdgcn_s_sleep(32);   // lazy x ~0.9 us
                } else {
                    if (ahead >= 64) __builtin_amdgcn_s_sleep(64);
                    else if (ahead >= 4) __builtin_amdgcn_s_sleep(8);
                }
            }
            s_item = it;
        }
        __syncthreads();
        const unsigned long long it = s_item;
        if (!it) return;
        const long long t_pick = wall_clock64();
        const unsigned long long *gp = reinterpret_cast<const unsigned long long *>(it);
        if (tid < kPktStride) pk[tid] = load_sys(gp + tid);
        __syncthreads();
        const int n_words = (int)(uni64(pk[12]) & 0xffffffffu);
        for (int w = kPktStride + tid; w < n_words && w < kPktWords; w += 128) pk[w] = load_sys(gp + w);
        // (records written by other workgroups of this kernel are read with agent-scope loads inside the body — an
        //  agent-scope acquire fence here would also drop the kernel's code and the poses from this XCD's L2 per item)
        __syncthreads();
        unsigned long long h[kPktHdr];
#pragma unroll
        for (int w = 0; w < kPktHdr; w++) h[w] = uni64(pk[w]);
        KArgs a;
        a.arena = reinterpret_cast<double *>(h[0]);
        a.mail = reinterpret_cast<double *>(h[1]);
        a.mail_base = (int64_t)h[2];
        a.blk = nullptr; a.vpo = nullptr; a.er = nullptr; a.ev = nullptr; a.list = nullptr; a.gws = nullptr; a.gws_stride = 0;
        a.algorithm = ALG == SPG_ALG_GLC ? SPG_ALG_GLC : SPG_ALG_NFR;
        a.topology = (int)(h[9] & 0xffffffffu); a.flags = (int)(h[9] >> 32);
        a.lin_point = (int)(h[10] & 0xffffffffu); a.tag = (int)(h[10] >> 32);
        a.chord_ratio = __longlong_as_double((long long)h[11]);
        spg_blanket_desc bd;
        bd.vert_begin = 0; bd.edge_begin = 0;
        bd.out_off = (int64_t)h[3]; bd.new_off = (int64_t)h[4]; bd.tinfo_off = (int64_t)h[5]; bd.new_len = 0;
        bd.n_vert = (int)(h[6] & 0xffffffffu); bd.n_remove = (int)(h[6] >> 32);
        bd.n_edge = (int)(h[7] & 0xffffffffu); bd.n_new_max = (int)(h[7] >> 32);
        bd.n_new_vert_max = (int)(h[8] & 0xffffffffu); bd.pad_ = (int)(h[8] >> 32);
        const int64_t *vpo = reinterpret_cast<const int64_t *>(pk + kPktHdr);
        const spg_edge_ref *er = reinterpret_cast<const spg_edge_ref *>(pk + kPktHdr + bd.n_vert);
        const int32_t *ev = reinterpret_cast<const int32_t *>(pk + kPktHdr + bd.n_vert + 3 * bd.n_edge);
        const long long t_body = wall_clock64();
        // inlined: as an out-of-line call the body saved / restored 56 callee-saved VGPRs per blanket through scratch —
        // 28 KB per workgroup and item, 1.3 GB of HBM writes per step of the bench workload (rocprofv3 WRITE_SIZE). Inlined
        // it needs the whole register file of a SIMD (256 VGPRs + ~110 AGPRs as spill space, no scratch): one wave per
        // SIMD, which is what a grid of one 2-wave workgroup per CU uses anyway.
        blanket_body<D, 128, false, ALG, true>(a, bd, vpo, er, ev, 0, smem);
        __syncthreads();
        if ((h[12] >> 32) & 0x40000000u) {
            // diagnostic (SPG_WORKER_STAMP=1): min_gap slot <- ticks to the ready word + 1e-6 * ticks to the final word, from the pick (100 MHz wall clock); the final
            // word is rewritten after it so that the host's late harvest sees the stamp
            if (tid == 0 && a.mail) {
                double *orec = a.mail + (bd.out_off - a.mail_base);
                const double *orl_ = smem + make_layout(D, 128, bd.n_vert - bd.n_remove, bd.n_remove, ALG, a.topology, bd.pad_).o_eO;
                orec[3] = (double)((long long)orl_[5] - t_pick) + 1e-6 * (double)(wall_clock64() - t_pick);   // ticks of 10 ns: ready, final
                __threadfence_system();
            }
        }
    }
}

}  // namespace

// =================================================================================== launch entry points
// What the backend (spg_hip_backend.cpp, host-only code) calls to put these kernels on a stream. Which variant, how many
// blocks and how much LDS is decided there (spg_round_plan.hpp); the timing events are the backend's as well.
namespace spg {

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { snprintf(err, errlen, "%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); return SPG_EHIP; } } while (0)

// (the worker first, then the blanket variants, then the pre-pass: the order the kernels have in the code object)
namespace {
template <int D>
int launch_worker(int grid, size_t lds, hipStream_t s, hipEvent_t ev_a, hipEvent_t ev_b, WorkQ *q, unsigned long long *ticket, long long idle_ticks,
                  int bells, int lazy, char *err, size_t errlen) {
    auto kern = blanket_worker<D, SPG_ALG_NFR>;
    if (lds > 48 * 1024)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipExtLaunchKernelGGL(kern, dim3(grid), dim3(128), (uint32_t)lds, s, ev_a, ev_b, 0, q, ticket, idle_ticks, bells, lazy);
    HIPCHK(hipGetLastError());
    return 0;
}
}  // namespace

int hip_worker_launch(int D, int grid, size_t lds_bytes, void *stream, void *ev_start, void *ev_stop, WorkQ *q, unsigned long long *ticket,
                      long long idle_ticks, int bells, int lazy, char *err, size_t errlen) {
    if (D == 6) return launch_worker<6>(grid, lds_bytes, (hipStream_t)stream, (hipEvent_t)ev_start, (hipEvent_t)ev_stop, q, ticket, idle_ticks, bells, lazy, err, errlen);
    if (D == 3) return launch_worker<3>(grid, lds_bytes, (hipStream_t)stream, (hipEvent_t)ev_start, (hipEvent_t)ev_stop, q, ticket, idle_ticks, bells, lazy, err, errlen);
    snprintf(err, errlen, "no worker kernel for D=%d", D);
    return SPG_EINVAL;
}

namespace {
template <int D, int NT, bool GWS, int ALG>
int launch_variant(hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop, const KArgs &ka, int nblocks, size_t lds_bytes, char *err, size_t errlen) {
    auto kern = blanket_kernel<D, NT, GWS, ALG>;
    if (lds_bytes > 64 * 1024)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    // one runtime call: the dispatch itself carries the two events (start / stop of this kernel)
    hipExtLaunchKernelGGL(kern, dim3(nblocks), dim3(NT), (uint32_t)lds_bytes, s, ev_start, ev_stop, 0, ka);
    HIPCHK(hipGetLastError());
    return 0;
}

// every instantiation of blanket_kernel there is, for both pose dimensions
struct VariantRow {
    BlanketVariant v;
    int (*launch)(hipStream_t, hipEvent_t, hipEvent_t, const KArgs &, int, size_t, char *, size_t);
};
#define SPG_VARIANT(NT, GWS, ALG) {{6, NT, GWS, ALG}, launch_variant<6, NT, GWS, ALG>}, {{3, NT, GWS, ALG}, launch_variant<3, NT, GWS, ALG>}
const VariantRow kVariants[] = {
    SPG_VARIANT(128, false, SPG_ALG_NFR_LM), SPG_VARIANT(128, false, SPG_ALG_NFR), SPG_VARIANT(256, false, SPG_ALG_NFR),
    SPG_VARIANT(64, false, SPG_ALG_GLC),     SPG_VARIANT(64, false, SPG_ALG_NFR_LM), SPG_VARIANT(64, false, SPG_ALG_NFR),
    SPG_VARIANT(256, true, SPG_ALG_GLC),     SPG_VARIANT(256, true, SPG_ALG_NFR_LM), SPG_VARIANT(1024, true, SPG_ALG_NFR),
    SPG_VARIANT(256, true, SPG_ALG_NFR),
};
#undef SPG_VARIANT
}  // namespace

int hip_blanket_launch(const BlanketVariant &v, void *stream, void *ev_start, void *ev_stop, const KArgs &ka, int nblocks, size_t lds_bytes,
                       char *err, size_t errlen) {
    for (const VariantRow &r : kVariants)
        if (r.v.D == v.D && r.v.NT == v.NT && r.v.gws == v.gws && r.v.alg == v.alg)
            return r.launch((hipStream_t)stream, (hipEvent_t)ev_start, (hipEvent_t)ev_stop, ka, nblocks, lds_bytes, err, errlen);
    snprintf(err, errlen, "no blanket kernel for D=%d with %d lanes, %s tiles, algorithm %d", v.D, v.NT, v.gws ? "workspace" : "LDS", v.alg);
    return SPG_EINVAL;
}

int hip_local_point_launch(int D, void *stream, int count, const double *arena, double *lpose, const spg_blanket_desc *blk, const int64_t *vpo,
                           const spg_edge_ref *er, const int32_t *ev, const int32_t *list, const int64_t *lp_off, int32_t *flag, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    if (D == 6) hipLaunchKernelGGL((local_point_kernel<6>), dim3((unsigned)count), dim3(64), 0, s, arena, lpose, blk, vpo, er, ev, list, lp_off, flag);
    else if (D == 3) hipLaunchKernelGGL((local_point_kernel<3>), dim3((unsigned)count), dim3(64), 0, s, arena, lpose, blk, vpo, er, ev, list, lp_off, flag);
    else { snprintf(err, errlen, "no local-point kernel for D=%d", D); return SPG_EINVAL; }
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace spg
