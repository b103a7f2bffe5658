// csrc/spg_blanket_layout.hpp — what the blanket kernels (spg_kernels.hip) and the host code that plans and launches
// them (spg_round_plan.hpp, spg_hip_backend.cpp) share: the LDS / workspace carve-up of one blanket, the kernel
// arguments and the set of kernel variants. Plain C++: a host compiler can include it.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/spg.h"

#if defined(__HIPCC__)
#define SPG_HOST_DEVICE __host__ __device__
#else
#define SPG_HOST_DEVICE
#endif

namespace spgdev {
// (largest target dimension n = d*k of the register-resident single-wavefront SPD kernels, spg_dev_wave.hpp)
// N = 36 would serve k <= 6 (SE3) too, but its 72 live fp64 registers push the whole kernel to 256
// VGPRs + scratch spills (rocprofv3: 8.3 MB of spill writes per 200-blanket launch); larger tiles use
// the LDS-cooperative routines instead.
constexpr int kWaveMax = 24;
}  // namespace spgdev

namespace spg {

constexpr int EC = 8;  // edges whose Jacobians are staged per chunk
// kernel-internal third value of the ALG template parameter: NFR with the blanket-level LM of the Local
// linearisation point compiled in (its pose-update arithmetic costs ~160 VGPRs; the plain NFR kernel has 84)
constexpr int SPG_ALG_NFR_LM = 2;

// LDS / workspace carve-up for one blanket (all offsets in doubles). Monotone in k and m, so the
// layout of the largest blanket of a launch bounds every blanket in it.
struct Layout {
    int n, nm, ld, ldm, P, NE;
    int o_pose, o_red, o_cs, o_ev, o_S, o_w, o_ldb, o_Lb, o_nJ, o_X, o_eJ, o_eO, o_eT, o_Ng, o_tre, o_xch, o_int, small_doubles;
    int o_M1, o_M2, o_M3, o_Hmm, o_Hmk, mat_doubles;
    // int area offsets (in ints, relative to o_int)
    int i_perm, i_keep, i_sorted, i_pij, i_comp, i_pairs, i_ev, i_misc, int_count;
    // GLC tail: CNT problems of size S (tree: k-1 of 2d; dense / k==1: one of n), see glc section
    int gS, gCNT, gld, gstride;
    int o_gmeas, o_gev, o_gcs, o_gscr;          // small (LDS)
    int i_gperm, i_gdone, i_gmeta, i_gverts;    // ints
    int o_G, o_gA;                              // mat space: 4 batch buffers; GLC-edge assembly scratch
};

#pragma GCC visibility push(hidden)   // (inline, shared between units for the first time: not a symbol of the library)
SPG_HOST_DEVICE inline Layout make_layout(int D, int nt, int k, int m, int alg = SPG_ALG_NFR, int topo = SPG_TOPO_TREE,
                                           int scratch = 0) {
    Layout L;
    const bool glc = (alg == SPG_ALG_GLC);
    const bool single = (topo == SPG_TOPO_DENSE) || k <= 1;
    int DD = D * D;
    L.n = D * k; L.nm = D * m;
    L.ld = L.n | 1; L.ldm = L.nm | 1;
    L.P = k * (k - 1) / 2;
    L.NE = k > 0 ? k : 1;  // most new edges any algorithm emits (GLC tree: root + k-1)
    int psz = (D == 6) ? 12 : 3;
    int o = 0;
    L.o_pose = o; o += (k + m) * psz;
    L.o_red = o; o += nt;
    L.o_cs = o; o += L.n + 4;
    L.o_ev = o; o += L.n;
    L.o_S = o; o += L.n;
    L.o_w = o; o += (L.P > 0 ? L.P : 1);
    L.o_ldb = o; o += k + 1;
    L.o_Lb = o; o += k * DD;
    L.o_nJ = o; o += L.NE * 2 * DD;
    L.o_X = o; o += L.NE * DD;
    L.o_eJ = o; o += EC * 2 * DD;
    L.o_eO = o; o += EC * DD;
    L.o_eT = o; o += EC * 2 * DD;
    L.o_Ng = o; o += L.n * D;
    L.o_tre = o; o += L.NE;
    L.o_xch = o; o += 4;
    L.gS = single ? (k > 0 ? D * k : D) : 2 * D;
    L.gCNT = single ? 1 : (k - 1);
    L.gld = L.gS | 1;
    L.gstride = L.gS * L.gld;
    L.o_gmeas = o; if (glc) o += L.gCNT * L.gS;
    L.o_gev = o; if (glc) o += L.gCNT * L.gS;
    L.o_gcs = o; if (glc) o += L.gCNT * (L.gS + 4);
    L.o_gscr = o; if (glc) o += L.gCNT * (2 * L.gS + 2);
    L.o_int = o;
    int io = 0;
    L.i_perm = io; io += L.n;
    L.i_keep = io; io += L.n;
    L.i_sorted = io; io += (L.P > 0 ? L.P : 1);
    L.i_pij = io; io += 2 * (L.P > 0 ? L.P : 1);
    L.i_comp = io; io += k + 1;
    L.i_pairs = io; io += 2 * L.NE;
    L.i_ev = io; io += 2 * EC;
    L.i_misc = io; io += 12;
    L.i_gperm = io; if (glc) io += L.gCNT * L.gS;
    L.i_gdone = io; if (glc) io += L.gCNT;
    L.i_gmeta = io; if (glc) io += 3 * (L.NE + 1);
    L.i_gverts = io; if (glc) io += 2 * L.NE + k + 2;
    L.int_count = io;
    o += (io + 1) / 2;
    L.small_doubles = o;
    int mo = 0;
    L.o_M1 = mo; mo += L.n * L.ld;
    L.o_M2 = mo; mo += L.n * L.ld;
    L.o_M3 = mo; mo += L.n * L.ld;
    L.o_Hmm = mo; mo += L.nm * L.ldm;
    L.o_Hmk = mo; mo += L.nm * L.ld;
    L.o_G = mo; if (glc) mo += 4 * L.gCNT * L.gstride;
    L.o_gA = mo; if (glc) mo += scratch;
    L.mat_doubles = mo;
    return L;
}
#pragma GCC visibility pop

struct KArgs {
    double *arena;
    const spg_blanket_desc *blk;
    const int64_t *vpo;
    const spg_edge_ref *er;
    const int32_t *ev;
    const int32_t *list;
    double *gws;
    int64_t gws_stride;
    int topology, algorithm, flags, lin_point, tag;
    double chord_ratio;
    double *mail;        // pinned host mailbox for out records (or nullptr)
    int64_t mail_base;   // arena offset that maps to mail[0]
};

// One instantiation of blanket_kernel: pose dimension, lanes per blanket, tiles in the global workspace (else LDS),
// algorithm (SPG_ALG_NFR, SPG_ALG_GLC or SPG_ALG_NFR_LM).
struct BlanketVariant {
    int D, NT;
    bool gws;
    int alg;
};

}  // namespace spg
