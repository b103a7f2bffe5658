// csrc/spg_sparse.inc — block-sparse multifrontal Cholesky on the device (SURVEY.md §8f.1), included by spg_dense.hip.
//
// Reference: the two places where the reference leaves dense linear algebra — optimize() (src/graph_wrapper_g2o.cpp:
// 250-269: g2o Levenberg-Marquardt over CHOLMOD) and the marginalisation inside kullbackLeibler()
// (src/graph_wrapper_g2o.cpp:531-548: Eigen::SimplicialLLT of H_mm, then DENSE n_g x n_g LDLT / solve — 720 GB at
// 100 k poses, i.e. infeasible there). CHOLMOD / SimplicialLLT are un-vendored third parties; this is a design of
// its own for one MI355X, checked against the dense path of this library (tests/test_sparse.py).
//
// Numeric phase for a plan of spg_sparse_plan.hpp. Every supernode owns a dense front [pivot | boundary]^2 in one
// pool in HBM (288 GB: the pool of the 100 k-pose KLD is 63 GB); fronts of one level of the assembly tree are
// independent and advance in lockstep, so a factorisation is a few hundred launches however many fronts there are:
//   * assembly: the global-KLD assembly kernel with a sink that puts block (v, u) into the front of u's supernode;
//   * extend-add of the children's Schur complements, one launch per child rank (fixed summation order);
//   * left-looking blocked partial Cholesky over 64-wide panels: column update (K = 64 p, accumulated in registers:
//     every tile of L is written once), diagonal tile in one wavefront (diag_potrf_body), panel = tile * L_pp^-T;
//   * the boundary block's Schur complement in one launch with K = NP.
// All tile products go through ONE item-driven kernel on the fp64 matrix cores (v_mfma_f64_16x16x4_f64, 64 x 64 tile
// per workgroup, 2 x 2 accumulators per wavefront); the host generates the item lists once per plan.
// Solves are multifrontal too (a front gathers its children's update vectors itself: no atomics, fixed order).
// For the global KLD the marginalised blocks are eliminated first, log det of the marginal comes from the kept
// supernodes' diagonals, and trace(Lambda_y^-1 Lambda_x) from the selected inverse (Takahashi recurrence, top-down
// over the kept fronts: Sigma_BB gathered from the parent, Y = L_BS L_SS^-1, Sigma_SB = -Y^T Sigma_BB,
// Sigma_SS = L_SS^-T L_SS^-1 - Sigma_SB Y) contracted with the sparsified graph's Hessian blocks edge by edge.
// Per-pose covariances run the same recurrence over every supernode of the graph's own plan and read the requested
// blocks out of the fronts (sp_sigma_blocks_kernel; per-vertex marginal KLD: sp_marginal_kld_kernel).
#include <cstdlib>
#include <cstring>
#include <memory>
#include <queue>
#include <unordered_map>
#include "spg_greedy_plan.hpp"

#include "spg_sparse_plan.hpp"

namespace {

using spg::sparse::Plan;

struct GemmItem {
    double *c;
    const double *a, *b;
    int32_t ldc, lda, ldb;
    int32_t aks, bks;     // element stride between successive K tiles of A / B
    int32_t nk, flags, pad_;
};
enum { GI_TA = 1, GI_TB = 2, GI_ACC = 4, GI_NEG = 8 };   // op(A) = A^T, op(B) = B^T, C += ..., ... -= sum

struct DiagItem {
    double *tile, *linv;
    int32_t ld, pad_;
};

struct EaPair {          // extend-add (child -> parent) and its reverse, the gather of Sigma_BB (parent -> child)
    double *child;       // child's boundary block
    double *parent;      // parent's front
    const int32_t *rel;  // scalar offset of each child boundary block inside the parent's front
    int32_t ldc, ldp, nrows, np_parent;
};

constexpr int SLD = 66;  // LDS row stride of a staged 64 x 64 tile

// C (op)= sum_k op(A_k) op(B_k), one 64 x 64 output tile per workgroup, four wavefronts with 2 x 2 MFMA blocks each.
__global__ __launch_bounds__(256) void sp_gemm_items_kernel(const GemmItem *items) {
    __shared__ double As[64 * SLD], Bs[64 * SLD];
    const GemmItem it = items[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = (w >> 1) * 32, c0 = (w & 1) * 32, li = lane & 15, lk = lane >> 4;
    const int srow = tid >> 2, scol = (tid & 3) * 16;
    const bool ta = it.flags & GI_TA, tb = it.flags & GI_TB;
    d4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int y = 0; y < 2; y++) acc[x][y] = d4{0, 0, 0, 0};
    // software pipeline: the global loads of K tile k + 1 are in flight while tile k is multiplied out of LDS
    double2 ra[8], rb[8];
    auto fetch = [&](int k) {
        const double *ga = it.a + (long long)k * it.aks + (long long)srow * it.lda + scol;
        const double *gb = it.b + (long long)k * it.bks + (long long)srow * it.ldb + scol;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            ra[i] = *reinterpret_cast<const double2 *>(ga + 2 * i);
            rb[i] = *reinterpret_cast<const double2 *>(gb + 2 * i);
        }
    };
    if (it.nk > 0) fetch(0);
    for (int k = 0; k < it.nk; k++) {
        if (k) __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; i++) {
            *reinterpret_cast<double2 *>(&As[srow * SLD + scol + 2 * i]) = ra[i];
            *reinterpret_cast<double2 *>(&Bs[srow * SLD + scol + 2 * i]) = rb[i];
        }
        __syncthreads();
        if (k + 1 < it.nk) fetch(k + 1);
#pragma unroll 4
        for (int k0 = 0; k0 < 64; k0 += 4) {
            double a[2], b[2];
#pragma unroll
            for (int x = 0; x < 2; x++) {
                const int rr = r0 + 16 * x + li, cc = c0 + 16 * x + li, kk = k0 + lk;
                a[x] = ta ? As[kk * SLD + rr] : As[rr * SLD + kk];     // op(A)[row][k]
                b[x] = tb ? Bs[cc * SLD + kk] : Bs[kk * SLD + cc];     // op(B)[k][col]
            }
#pragma unroll
            for (int x = 0; x < 2; x++)
#pragma unroll
                for (int y = 0; y < 2; y++) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[x][y], 0, 0, 0);
        }
    }
    const bool accum = it.flags & GI_ACC, neg = it.flags & GI_NEG;
    // C/D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int y = 0; y < 2; y++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = r0 + 16 * x + lk + 4 * r, col = c0 + 16 * y + li;
                double *dst = it.c + (long long)row * it.ldc + col;
                const double v = neg ? -acc[x][y][r] : acc[x][y][r];
                *dst = accum ? (*dst + v) : v;
            }
}

__global__ __launch_bounds__(64) void sp_diag_items_kernel(const DiagItem *items, int *bad) {
    __shared__ double Ls[TB * 65], Li[TB * 65];
    const DiagItem it = items[blockIdx.x];
    diag_potrf_body(Ls, Li, it.tile, it.ld, it.linv, bad, 1);
}

// parent front += child's Schur complement (lower block triangle; diagonal d x d blocks in full). One wavefront per
// child block row; blockIdx.x = pair, blockIdx.y * 4 + wave = block row.
template <int D>
__global__ __launch_bounds__(256) void sp_extend_add_kernel(const EaPair *pairs) {
    const EaPair pr = pairs[blockIdx.x];
    const int t1 = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t1 >= pr.nrows) return;
    const int r1 = pr.rel[t1];
    for (int cc = lane; cc < D * (t1 + 1); cc += 64) {
        const int t2 = cc / D, c = cc - t2 * D;
        const int dcol = pr.rel[t2] + c;
#pragma unroll
        for (int r = 0; r < D; r++) {
            double *dst = pr.parent + (long long)(r1 + r) * pr.ldp + dcol;
            *dst += pr.child[(long long)(D * t1 + r) * pr.ldc + cc];
        }
    }
}

// child's Sigma_BB (full, symmetric) <- parent's Sigma front. The parent's front holds Sigma_SS (full), Sigma_SB in the
// upper right block and Sigma_BB (full); its lower left block still holds Y, so entries there are read transposed.
template <int D>
__global__ __launch_bounds__(256) void sp_gather_sigma_kernel(const EaPair *pairs) {
    const EaPair pr = pairs[blockIdx.x];
    const int t1 = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t1 >= pr.nrows) return;
    const int r1 = pr.rel[t1];
    for (int cc = lane; cc < D * pr.nrows; cc += 64) {
        const int t2 = cc / D, c = cc - t2 * D;
        const int pc = pr.rel[t2] + c;
#pragma unroll
        for (int r = 0; r < D; r++) {
            const int prow = r1 + r;
            const double v = (prow >= pr.np_parent && pc < pr.np_parent) ? pr.parent[(long long)pc * pr.ldp + prow]
                                                                         : pr.parent[(long long)prow * pr.ldp + pc];
            pr.child[(long long)(D * t1 + r) * pr.ldc + cc] = v;
        }
    }
}

struct SpDev {           // device view of a plan
    double *pool, *linv, *work;
    const int32_t *first, *rowptr, *rows, *rel, *childptr, *child, *NP, *NB, *sn_of, *level_sn;
    const int64_t *foff, *loff, *woff;
    int D, nsn;
};

// Pivot diagonals of every front: += lambda on the real unknowns, 1 on the pad; partial[s] = max |diag| before the shift
__global__ __launch_bounds__(64) void sp_diag_shift_kernel(SpDev P, double lambda, double *partial) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int ld = P.NP[s] + P.NB[s], ns = P.D * (P.first[s + 1] - P.first[s]);
    double *F = P.pool + P.foff[s];
    double m = 0;
    for (int i = lane; i < P.NP[s]; i += 64) {
        double *d = F + (long long)i * ld + i;
        if (i < ns) { m = fmax(m, fabs(*d)); *d += lambda; }
        else *d = 1.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if (partial && lane == 0) partial[s] = m;
}

__global__ __launch_bounds__(256) void sp_max_kernel(const double *v, int n, double *out, int slot) {
    __shared__ double red[256];
    double s = 0;
    for (int i = threadIdx.x; i < n; i += 256) s = fmax(s, v[i]);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[slot] = red[0];
}

// partial[s] = sum_{i < ns} log L_ii of front s
__global__ __launch_bounds__(64) void sp_logdiag_kernel(SpDev P, double *partial) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int ld = P.NP[s] + P.NB[s], ns = P.D * (P.first[s + 1] - P.first[s]);
    const double *F = P.pool + P.foff[s];
    double m = 0;
    for (int i = lane; i < ns; i += 64) m += log(F[(long long)i * ld + i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
    if (lane == 0) partial[s] = m;
}

// L y = x in place, one workgroup per front of one level (blockIdx.x indexes level_sn from lbegin): the front's local
// vector = its pivot entries of x + the update vectors of its children (gathered in child order), forward substitution
// over the pivot tiles, the boundary part of the local vector is the update vector handed to the parent.
__global__ __launch_bounds__(1024) void sp_forward_kernel(SpDev P, int lbegin, double *x) {
    __shared__ double xs[64], rs[64];
    const int s = P.level_sn[lbegin + blockIdx.x], tid = threadIdx.x, D = P.D, nt = blockDim.x;
    const int np = P.NP[s], ld = np + P.NB[s], ns = D * (P.first[s + 1] - P.first[s]), base = D * P.first[s];
    double *r = P.work + P.woff[s];
    for (int i = tid; i < ld; i += nt) r[i] = (i < ns) ? x[base + i] : 0.0;
    __syncthreads();
    for (int ci = P.childptr[s]; ci < P.childptr[s + 1]; ci++) {
        const int c = P.child[ci], nrc = P.rowptr[c + 1] - P.rowptr[c];
        const double *uc = P.work + P.woff[c] + P.NP[c];
        const int32_t *relc = P.rel + P.rowptr[c];
        for (int idx = tid; idx < nrc * D; idx += nt) {
            const int t = idx / D, d = idx - t * D;
            r[relc[t] + d] += uc[idx];
        }
        __syncthreads();
    }
    const double *F = P.pool + P.foff[s], *Li = P.linv + P.loff[s];
    for (int p = 0; p < np / 64; p++) {
        if (tid < 64) rs[tid] = r[64 * p + tid];
        __syncthreads();
        if (tid < 64) {
            const double *row = Li + (long long)p * 4096 + tid * 64;
            double acc = 0;
            for (int c = 0; c <= tid; c++) acc += row[c] * rs[c];
            xs[tid] = acc;
            r[64 * p + tid] = acc;
        }
        __syncthreads();
        for (int i = 64 * (p + 1) + tid; i < ld; i += nt) {
            const double *row = F + (long long)i * ld + 64 * p;
            double u = 0;
#pragma unroll 8
            for (int c = 0; c < 64; c++) u += row[c] * xs[c];
            r[i] -= u;
        }
        __syncthreads();
    }
    for (int i = tid; i < ns; i += nt) x[base + i] = r[i];
}

// L^T x = y in place, levels descending: boundary values are the already solved unknowns of the ancestors.
// mode 1: no solve — z = L^T x of the front's columns, partial[s] = sum z_j^2 (Mahalanobis term), x untouched.
__global__ __launch_bounds__(1024) void sp_backward_kernel(SpDev P, int lbegin, double *x, int mode, double *partial) {
    __shared__ double red[16][64], vs[64];
    const int s = P.level_sn[lbegin + blockIdx.x], tid = threadIdx.x, D = P.D, nt = blockDim.x, ng = nt >> 6;
    const int np = P.NP[s], ld = np + P.NB[s], ns = D * (P.first[s + 1] - P.first[s]), base = D * P.first[s];
    const int nr = P.rowptr[s + 1] - P.rowptr[s];
    double *r = P.work + P.woff[s];
    for (int i = tid; i < np; i += nt) r[i] = (i < ns) ? x[base + i] : 0.0;
    for (int i = tid; i < ld - np; i += nt) {
        const int t = i / D, d = i - t * D;
        r[np + i] = (t < nr) ? x[D * P.rows[P.rowptr[s] + t] + d] : 0.0;
    }
    __syncthreads();
    const double *F = P.pool + P.foff[s], *Li = P.linv + P.loff[s];
    const int g = tid >> 6, j = tid & 63;
    double zz = 0;
    for (int p = np / 64 - 1; p >= 0; p--) {
        double acc = 0;
        const int ibeg = (mode == 1) ? 64 * p : 64 * (p + 1);
        for (int i = ibeg + g; i < ld; i += ng) acc += F[(long long)i * ld + 64 * p + j] * r[i];
        red[g][j] = acc;
        __syncthreads();
        if (mode == 1) {
            if (g == 0) { double z = 0; for (int w = 0; w < ng; w++) z += red[w][j]; if (64 * p + j < ns) zz += z * z; }
            __syncthreads();
            continue;
        }
        if (g == 0) { double z = 0; for (int w = 0; w < ng; w++) z += red[w][j]; vs[j] = r[64 * p + j] - z; }
        __syncthreads();
        if (g == 0) {
            const double *col = Li + (long long)p * 4096 + j;
            double a2 = 0;
            for (int i = j; i < 64; i++) a2 += col[i * 64] * vs[i];
            r[64 * p + j] = a2;
        }
        __syncthreads();
    }
    if (mode == 1) {
        if (g == 0) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) zz += __shfl_xor(zz, o, 64);
            if (j == 0) partial[s] = zz;
        }
        return;
    }
    for (int i = tid; i < ns; i += nt) x[base + i] = r[i];
}

// out[pos[i] + d] = in[i * D + d]: a per-vertex vector into elimination order
__global__ void scatter_blocks_kernel(const double *in, const int32_t *pos, int n, int D, double *out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * D) return;
    const int i = idx / D, d = idx - i * D;
    out[pos[i] + d] = in[idx];
}

// identity on the diagonal of every kept front's Z block (the pool was zeroed)
__global__ void sp_z_identity_kernel(double *zpool, const int64_t *zoff, const int32_t *NPv, const int32_t *list, int n) {
    const int s = list[blockIdx.x];
    double *Z = zpool + zoff[s];
    const int np = NPv[s];
    for (int i = threadIdx.x; i < np; i += blockDim.x) Z[(long long)i * np + i] = 1.0;
}

// Sink of the assembly kernel that writes into the fronts: block (row v, column u), pos(u) < pos(v), lives in the front
// of u's supernode — among its pivot rows when v is a column of the same supernode, else at v's boundary row.
struct FrontSink {
    SpDev P;
    int *bad;
    __device__ __forceinline__ double *locate(int pv, int pu, int &ld, bool &transposed, bool sigma) const {
        const int D = P.D, qu = pu / D, qv = pv / D, s = P.sn_of[qu];
        const int np = P.NP[s];
        ld = np + P.NB[s];
        double *F = P.pool + P.foff[s];
        const int col = pu - D * P.first[s];
        transposed = false;
        if (qv < P.first[s + 1]) return F + (long long)(pv - D * P.first[s]) * ld + col;
        int lo = P.rowptr[s], hi = P.rowptr[s + 1] - 1, at = -1;
        while (lo <= hi) {
            const int mid = (lo + hi) >> 1, q = P.rows[mid];
            if (q == qv) { at = mid; break; }
            if (q < qv) lo = mid + 1; else hi = mid - 1;
        }
        if (at < 0) { *bad = 2; return nullptr; }
        const int row = np + D * (at - P.rowptr[s]);
        if (sigma) { transposed = true; return F + (long long)col * ld + row; }   // Sigma_SB: [column][boundary row]
        return F + (long long)row * ld + col;
    }
    __device__ __forceinline__ void add(int pv, int pu, int r, int c, double val) {
        int ld; bool tr;
        double *blk = locate(pv, pu, ld, tr, false);
        if (blk) blk[(long long)r * ld + c] += val;
    }
    __device__ __forceinline__ void diag(int pv, int r, int c, double val) {
        const int D = P.D, s = P.sn_of[pv / D], ld = P.NP[s] + P.NB[s], o = pv - D * P.first[s];
        P.pool[P.foff[s] + (long long)(o + r) * ld + o + c] = val;
    }
    __device__ __forceinline__ void finish(int, int) {}
};

// Sink that contracts the assembled blocks with the selected inverse held in the fronts:
// partial[v] = sum over the blocks the assembly would write for vertex v of <block, Sigma block> (off-diagonal
// blocks twice) — summed over v this is trace(Sigma H).
struct TraceSink {
    FrontSink fs;
    double *partial;
    double acc;
    __device__ __forceinline__ void add(int pv, int pu, int r, int c, double val) {
        int ld; bool tr;
        const double *blk = fs.locate(pv, pu, ld, tr, true);
        if (blk) acc += 2.0 * val * (tr ? blk[(long long)c * ld + r] : blk[(long long)r * ld + c]);
    }
    __device__ __forceinline__ void diag(int pv, int r, int c, double val) {
        const SpDev &P = fs.P;
        const int D = P.D, s = P.sn_of[pv / D], ld = P.NP[s] + P.NB[s], o = pv - D * P.first[s];
        acc += val * P.pool[P.foff[s] + (long long)(o + r) * ld + o + c];
    }
    __device__ __forceinline__ void finish(int v, int tid) {
        double a = acc;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (tid == 0) partial[v] = a;
    }
};

// Covariance blocks out of the selected inverse held in the fronts. Request i names K vertices by their positions
// (D * elimination position; -1 = the fixed vertex, whose rows and columns are zero) and gets the (K D) x (K D) block
// [Sigma(v_a, v_b)]_ab row-major at out + i (K D)^2. One wavefront per request; each D x D sub-block is read through
// FrontSink::locate with pos(u) <= pos(v) (Sigma_SB is stored transposed; the lower-left block of a front still holds Y
// and is never read), the upper sub-blocks by symmetry. Only real rows and columns are addressed, never the pads.
// A sub-block outside the fronts sets bad = 2 and reads as zero.
template <int D, int K>
__global__ __launch_bounds__(64) void sp_sigma_blocks_kernel(FrontSink fs, const int32_t *req, int n, double *out) {
    constexpr int W = K * D;
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const int32_t *p = req + (long long)i * K;
    double *o = out + (long long)i * W * W;
    for (int e = lane; e < W * W; e += 64) {
        const int a = e / W, b = e - a * W, ka = a / D, kb = b / D, r = a - ka * D, c = b - kb * D;
        const int pa = p[ka], pb = p[kb];
        double v = 0.0;
        if (pa >= 0 && pb >= 0) {
            const bool lower = pa >= pb;
            const int pv = lower ? pa : pb, pu = lower ? pb : pa, rr = lower ? r : c, cc = lower ? c : r;
            int ld; bool tr;
            const double *blk = fs.locate(pv, pu, ld, tr, true);
            if (blk) v = tr ? blk[(long long)cc * ld + rr] : blk[(long long)rr * ld + cc];
        }
        o[e] = v;
    }
}

// ---- columns of Sigma by multi-right-hand-side solves through the fronts (spg_graph_pair_covariances and
// spg_graph_joint_marginal_covariance). A batch solves R right-hand sides (D identity columns per column vertex) over
// the union of the root paths it needs; every touched front s owns a row-major ld(s) x R panel in one workspace. The
// tile products of the sweeps are items of sp_gemm_items_kernel; the kernels below move panel rows between fronts.
struct PanelPair {       // child <-> parent panel rows: child boundary row t <-> parent row rel[t / D] + t % D
    double *child;       // the child's panel at its first boundary row
    double *parent;      // the parent's panel
    const int32_t *rel;
    int32_t nrows;       // child boundary rows in scalars
    int32_t R;           // panel width
};

// GATHER = false: parent rows += child's update rows (forward; one launch per child rank, fixed order).
// GATHER = true: child's boundary rows <- the parent's solved unknowns (backward). blockIdx = (pair, 64-column tile,
// 64-row chunk), four wavefronts of 16 rows each; lane = column. Every destination element has one writer per launch.
template <int D, bool GATHER>
__global__ __launch_bounds__(256) void sp_panel_rows_kernel(const PanelPair *pairs) {
    const PanelPair pr = pairs[blockIdx.x];
    const int col = blockIdx.y * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;
    for (int k = 0; k < 16; k++) {
        const int t = blockIdx.z * 64 + w * 16 + k;
        if (t >= pr.nrows) return;
        const int q = t / D;
        double *c = pr.child + (long long)t * pr.R + col;
        double *p = pr.parent + (long long)(pr.rel[q] + t - q * D) * pr.R + col;
        if (GATHER) *c = *p;
        else *p += *c;
    }
}

// ws[at[i]] = 1: the identity columns of a batch's column vertices, in their fronts' pivot rows
__global__ void sp_panel_seed_kernel(double *ws, const int64_t *at, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ws[at[i]] = 1.0;
}

// cross[dst[i] D^2 + r D + c] = ws[src[i] + r R + c]: the solved rows of request i (D x D, row-major)
__global__ void sp_cross_rows_kernel(const double *ws, const int64_t *src, const int32_t *dst, int n, int D, int R, double *cross) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * D * D) return;
    const int i = idx / (D * D), e = idx - i * D * D, r = e / D, c = e - r * D;
    cross[(long long)dst[i] * D * D + e] = ws[src[i] + (long long)r * R + c];
}

// One D x D output sub-block of a pair / set covariance: out[dst + r ld + c]. cross >= 0: from the solved cross blocks
// (transposed when the solved column was the other vertex); else pa, pb >= 0: from the selected inverse in the fronts,
// read as sp_sigma_blocks_kernel reads it; else zero (the fixed vertex).
struct CovBlk {
    int64_t dst;
    int32_t ld, pa, pb, cross, tr, pad_;
};
template <int D>
__global__ __launch_bounds__(256) void sp_cov_assemble_kernel(FrontSink fs, const CovBlk *blks, int n, const double *cross, double *out) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n || lane >= D * D) return;
    const CovBlk b = blks[i];
    const int r = lane / D, c = lane - r * D;
    double v = 0.0;
    if (b.cross >= 0) {
        v = cross[(long long)b.cross * D * D + (b.tr ? c * D + r : r * D + c)];
    } else if (b.pa >= 0 && b.pb >= 0) {
        const bool lower = b.pa >= b.pb;
        const int pv = lower ? b.pa : b.pb, pu = lower ? b.pb : b.pa, rr = lower ? r : c, cc = lower ? c : r;
        int ld; bool tr;
        const double *blk = fs.locate(pv, pu, ld, tr, true);
        if (blk) v = tr ? blk[(long long)cc * ld + rr] : blk[(long long)rr * ld + cc];
    }
    out[b.dst + (long long)r * b.ld + c] = v;
}

// Relative-pose covariances and candidate-edge scores (spg_graph_relative_covariances / spg_graph_score_candidates) from
// the assembled pair blocks, which stay on the device. Candidate i is a hypothetical binary edge a -> b: vertex indices
// va[i], vb[i] (their poses, the fixed vertex included), slot[i] = its 2D x 2D block Sigma_ab in `blocks` (shared by
// every candidate of one pair) and, when rec != nullptr, its record (measurement + upper triangle of Omega, the layout of
// spg_graph_add_edges). With J = [Ja Jb] of se2_edge_jac / se3_edge_jac at the measurement z: P = J Sigma_ab J^T.
//   rec == nullptr  z = the current relative pose (se2_between; Xa^-1 Xb): writes rel (t + quaternion, may be nullptr)
//                   and P (r <= c computed, mirrored: exactly symmetric) into cov;
//   rec != nullptr  Omega = L L^T, M = I + L^T P L = G G^T (M >= I: cannot fail for finite P), y = L^T e:
//                   chi2 = e^T Omega e, d2 = || G^-1 y ||^2 = e^T (P + Omega^-1)^-1 e, gain = sum log G_jj = 1/2 ln det M;
//                   Omega not finite or not PD: status 1 (SPG_CAND_INFO_NOT_PD) and three NaN, else status 0.
// One wavefront per candidate, four per workgroup; Sigma_ab, J, J Sigma_ab, P, L and M in the wavefront's LDS slice
// (372 doubles for D = 6). The geometry and the two D x D factorisations run on lane 0, the products over the lanes.
struct RelArgs {
    const double *arena;
    const int64_t *vpo;       // per vertex index: pose offset in the arena
    const int32_t *va, *vb, *slot;
    const double *rec;        // n x (PS + D (D + 1) / 2) or nullptr
    const double *blocks;     // per slot (2D)^2, row-major
    double *rel, *cov;        // relative mode
    double *score;            // score mode: d2[n], gain[n], chi2[n]
    int32_t *status;
    int n;
};
template <int D>
__global__ __launch_bounds__(256) void sp_relative_kernel(RelArgs a) {
    constexpr int W = 2 * D, DD = D * D, PS = (D == 6) ? 7 : 3, PSZ = (D == 6) ? kIso : 3, TRI = D * (D + 1) / 2, REC = PS + TRI;
    constexpr int PER = W * W + 2 * DD + D * W + 2 * DD + 2 * D;
    __shared__ double lds[4 * PER];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = blockIdx.x * 4 + w;
    const bool act = i < a.n;
    double *S = lds + w * PER, *Ja = S + W * W, *Jb = Ja + DD, *T = Jb + DD, *P = T + D * W, *L = P + DD, *e = L + DD, *y = e + D;
    double *A = T, *M = T + DD;   // score mode: P L and M reuse J Sigma_ab once P is formed
    const bool score = a.rec != nullptr;
    const double *rec = score && act ? a.rec + (long long)i * REC : nullptr;
    if (act) {
        const double *blk = a.blocks + (long long)a.slot[i] * W * W;
        for (int k = lane; k < W * W; k += 64) S[k] = blk[k];
        if (lane == 0) {
            double Xa[PSZ], Xb[PSZ], err[D];
            load_pose<D>(a.arena, a.vpo[a.va[i]], Xa);
            load_pose<D>(a.arena, a.vpo[a.vb[i]], Xb);
            if (D == 6) {
                double Z[kIso];
                if (score) {
                    iso_from_tq(rec, Z);
                } else {
                    iso_inv_mul(Xa, Xb, Z);
                    if (a.rel) {
                        double q[4];
                        R_to_quat(Z, q);
                        double *o = a.rel + (long long)i * PS;
                        o[0] = Z[9]; o[1] = Z[10]; o[2] = Z[11]; o[3] = q[0]; o[4] = q[1]; o[5] = q[2]; o[6] = q[3];
                    }
                }
                se3_edge_jac(Xa, Xb, Z, Ja, Jb, err);
            } else {
                double z[3];
                if (score) { z[0] = rec[0]; z[1] = rec[1]; z[2] = rec[2]; }
                else {
                    se2_between(Xa, Xb, z);
                    if (a.rel) { double *o = a.rel + (long long)i * PS; o[0] = z[0]; o[1] = z[1]; o[2] = z[2]; }
                }
                se2_edge_jac(Xa, Xb, z, Ja, Jb, err);
            }
#pragma unroll
            for (int k = 0; k < D; k++) e[k] = err[k];
        }
    }
    __syncthreads();
    if (act)   // T = J Sigma_ab (D x 2D)
        for (int k = lane; k < D * W; k += 64) {
            const int r = k / W, c = k - r * W;
            double s = 0;
            for (int t = 0; t < D; t++) s += Ja[r * D + t] * S[t * W + c];
            for (int t = 0; t < D; t++) s += Jb[r * D + t] * S[(D + t) * W + c];
            T[k] = s;
        }
    __syncthreads();
    if (act && lane < DD) {   // P = T J^T, r <= c, mirrored
        const int r = lane / D, c = lane - r * D;
        if (r <= c) {
            double s = 0;
            for (int t = 0; t < D; t++) s += T[r * W + t] * Ja[c * D + t];
            for (int t = 0; t < D; t++) s += T[r * W + D + t] * Jb[c * D + t];
            P[r * D + c] = s;
            P[c * D + r] = s;
            if (!score) {
                a.cov[(long long)i * DD + r * D + c] = s;
                a.cov[(long long)i * DD + c * D + r] = s;
            }
        }
    }
    if (!score) return;
    __shared__ int okv[4];
    if (act && lane == 0) {   // Omega = L L^T in place (lower triangle; the upper is zeroed), chi2, y = L^T e
        bool ok = true;
        double chi = 0;
        int p = PS;
        for (int r = 0; r < D; r++)
            for (int c = r; c < D; c++) {
                const double v = rec[p++];
                ok = ok && isfinite(v);
                chi += ((r == c) ? 1.0 : 2.0) * e[r] * v * e[c];
                L[c * D + r] = v;
                if (c > r) L[r * D + c] = 0.0;
            }
        for (int j = 0; j < D && ok; j++) {
            double d = L[j * D + j];
            for (int k = 0; k < j; k++) d -= L[j * D + k] * L[j * D + k];
            ok = d > 0.0 && isfinite(d);
            if (!ok) break;
            d = sqrt(d);
            L[j * D + j] = d;
            for (int r = j + 1; r < D; r++) {
                double v = L[r * D + j];
                for (int k = 0; k < j; k++) v -= L[r * D + k] * L[j * D + k];
                L[r * D + j] = v / d;
            }
        }
        okv[w] = ok;
        if (ok) {
            for (int c = 0; c < D; c++) {
                double s = 0;
                for (int r = c; r < D; r++) s += L[r * D + c] * e[r];
                y[c] = s;
            }
            a.score[2LL * a.n + i] = chi;
            a.status[i] = 0;
        } else {
            const double nan = __builtin_nan("");
            a.score[i] = nan; a.score[(long long)a.n + i] = nan; a.score[2LL * a.n + i] = nan;
            a.status[i] = 1;
        }
    }
    __syncthreads();
    const bool go = act && okv[w];
    if (go && lane < DD) {   // A = P L
        const int r = lane / D, c = lane - r * D;
        double s = 0;
        for (int t = c; t < D; t++) s += P[r * D + t] * L[t * D + c];
        A[lane] = s;
    }
    __syncthreads();
    if (go && lane < DD) {   // M = I + L^T A, r <= c, mirrored
        const int r = lane / D, c = lane - r * D;
        if (r <= c) {
            double s = (r == c) ? 1.0 : 0.0;
            for (int t = r; t < D; t++) s += L[t * D + r] * A[t * D + c];
            M[r * D + c] = s;
            M[c * D + r] = s;
        }
    }
    __syncthreads();
    if (go && lane == 0) {   // M = G G^T in place, forward solve G x = y
        double gain = 0, d2 = 0;
        for (int j = 0; j < D; j++) {
            double d = M[j * D + j];
            for (int k = 0; k < j; k++) d -= M[j * D + k] * M[j * D + k];
            d = sqrt(d);
            M[j * D + j] = d;
            gain += log(d);
            for (int r = j + 1; r < D; r++) {
                double v = M[r * D + j];
                for (int k = 0; k < j; k++) v -= M[r * D + k] * M[j * D + k];
                M[r * D + j] = v / d;
            }
            double x = y[j];
            for (int k = 0; k < j; k++) x -= M[j * D + k] * y[k];
            x /= d;
            y[j] = x;
            d2 += x * x;
        }
        a.score[i] = d2;
        a.score[(long long)a.n + i] = gain;
    }
}

// The steps of sp_relative_kernel as functions, for the selection kernels below. Each is one wavefront's work between two
// barriers over its own LDS slice; "lane 0" steps are called by that lane alone. sp_relative_kernel itself keeps its own
// text: built from these functions (or as one body shared with sp_select_init_kernel) its SE3 results moved in the last
// bits (P by up to 2.7e-12 relative: other fused multiply-adds in the inlined geometry), and the existing calls return the
// bits they returned before. A change to the arithmetic of one has to be made in the other.
// lane 0: the poses of vertices va, vb, the measurement (rec, or the current relative pose, written to rel if given), the
// Jacobians and the error
template <int D>
__device__ __forceinline__ void rel_geometry(const double *arena, const int64_t *vpo, int32_t va, int32_t vb, const double *rec, double *rel, double *Ja,
                                             double *Jb, double *e) {
    constexpr int PSZ = (D == 6) ? kIso : 3;
    double Xa[PSZ], Xb[PSZ], err[D];
    load_pose<D>(arena, vpo[va], Xa);
    load_pose<D>(arena, vpo[vb], Xb);
    if (D == 6) {
        double Z[kIso];
        if (rec) {
            iso_from_tq(rec, Z);
        } else {
            iso_inv_mul(Xa, Xb, Z);
            if (rel) {
                double q[4];
                R_to_quat(Z, q);
                rel[0] = Z[9]; rel[1] = Z[10]; rel[2] = Z[11]; rel[3] = q[0]; rel[4] = q[1]; rel[5] = q[2]; rel[6] = q[3];
            }
        }
        se3_edge_jac(Xa, Xb, Z, Ja, Jb, err);
    } else {
        double z[3];
        if (rec) { z[0] = rec[0]; z[1] = rec[1]; z[2] = rec[2]; }
        else {
            se2_between(Xa, Xb, z);
            if (rel) { rel[0] = z[0]; rel[1] = z[1]; rel[2] = z[2]; }
        }
        se2_edge_jac(Xa, Xb, z, Ja, Jb, err);
    }
#pragma unroll
    for (int k = 0; k < D; k++) e[k] = err[k];
}
// T = [Ja Jb] S (D x 2D), S a 2D x 2D block
template <int D>
__device__ __forceinline__ void rel_J_sigma(int lane, const double *Ja, const double *Jb, const double *S, double *T) {
    constexpr int W = 2 * D;
    for (int k = lane; k < D * W; k += 64) {
        const int r = k / W, c = k - r * W;
        double s = 0;
        for (int t = 0; t < D; t++) s += Ja[r * D + t] * S[t * W + c];
        for (int t = 0; t < D; t++) s += Jb[r * D + t] * S[(D + t) * W + c];
        T[k] = s;
    }
}
// lanes < D^2: P = T [Ja Jb]^T, r <= c, mirrored; also into cov if given
template <int D>
__device__ __forceinline__ void rel_P(int lane, const double *T, const double *Ja, const double *Jb, double *P, double *cov) {
    constexpr int W = 2 * D;
    const int r = lane / D, c = lane - r * D;
    if (r <= c) {
        double s = 0;
        for (int t = 0; t < D; t++) s += T[r * W + t] * Ja[c * D + t];
        for (int t = 0; t < D; t++) s += T[r * W + D + t] * Jb[c * D + t];
        P[r * D + c] = s;
        P[c * D + r] = s;
        if (cov) {
            cov[r * D + c] = s;
            cov[c * D + r] = s;
        }
    }
}
// lane 0: Omega (info: its upper triangle) = L L^T in place (lower triangle; the upper is zeroed), chi = e^T Omega e and,
// when Omega is finite and positive definite (the return value), y = L^T e
template <int D>
__device__ __forceinline__ bool rel_omega(const double *info, const double *e, double *L, double *y, double &chi_out) {
    bool ok = true;
    double chi = 0;
    int p = 0;
    for (int r = 0; r < D; r++)
        for (int c = r; c < D; c++) {
            const double v = info[p++];
            ok = ok && isfinite(v);
            chi += ((r == c) ? 1.0 : 2.0) * e[r] * v * e[c];
            L[c * D + r] = v;
            if (c > r) L[r * D + c] = 0.0;
        }
    for (int j = 0; j < D && ok; j++) {
        double d = L[j * D + j];
        for (int k = 0; k < j; k++) d -= L[j * D + k] * L[j * D + k];
        ok = d > 0.0 && isfinite(d);
        if (!ok) break;
        d = sqrt(d);
        L[j * D + j] = d;
        for (int r = j + 1; r < D; r++) {
            double v = L[r * D + j];
            for (int k = 0; k < j; k++) v -= L[r * D + k] * L[j * D + k];
            L[r * D + j] = v / d;
        }
    }
    if (ok)
        for (int c = 0; c < D; c++) {
            double s = 0;
            for (int r = c; r < D; r++) s += L[r * D + c] * e[r];
            y[c] = s;
        }
    chi_out = chi;
    return ok;
}
// lanes < D^2: A = P L (L lower triangular)
template <int D>
__device__ __forceinline__ void rel_PL(int lane, const double *P, const double *L, double *A) {
    const int r = lane / D, c = lane - r * D;
    double s = 0;
    for (int t = c; t < D; t++) s += P[r * D + t] * L[t * D + c];
    A[lane] = s;
}
// lanes < D^2: M = I + L^T A, r <= c, mirrored
template <int D>
__device__ __forceinline__ void rel_M(int lane, const double *L, const double *A, double *M) {
    const int r = lane / D, c = lane - r * D;
    if (r <= c) {
        double s = (r == c) ? 1.0 : 0.0;
        for (int t = r; t < D; t++) s += L[t * D + r] * A[t * D + c];
        M[r * D + c] = s;
        M[c * D + r] = s;
    }
}
// lane 0: M = G G^T in place (lower triangle) with the forward solve G x = y interleaved (x replaces y):
// gain = sum log G_jj, d2 = || x ||^2
template <int D>
__device__ __forceinline__ void rel_chol_M(double *M, double *y, double &gain_out, double &d2_out) {
    double gain = 0, d2 = 0;
    for (int j = 0; j < D; j++) {
        double d = M[j * D + j];
        for (int k = 0; k < j; k++) d -= M[j * D + k] * M[j * D + k];
        d = sqrt(d);
        M[j * D + j] = d;
        gain += log(d);
        for (int r = j + 1; r < D; r++) {
            double v = M[r * D + j];
            for (int k = 0; k < j; k++) v -= M[r * D + k] * M[j * D + k];
            M[r * D + j] = v / d;
        }
        double x = y[j];
        for (int k = 0; k < j; k++) x -= M[j * D + k] * y[k];
        x /= d;
        y[j] = x;
        d2 += x * x;
    }
    gain_out = gain;
    d2_out = d2;
}

// Greedy selection of candidate edges by conditional information gain (spg_graph_select_candidates, DESIGN 5g-S). The
// joint covariance of the m distinct non-fixed endpoints (m D x m D, row-major) stays on the device; candidate i is the
// edge va[i] -> vb[i] (vertex indices: the poses) whose endpoints sit at block slots sa[i], sb[i] of the joint block
// (-1 = the fixed vertex: zero blocks). With C_ij = J_i Sigma_(ai bi),(aj bj) J_j^T, round t picks i* = argmax of
// gain_i = 1/2 ln det(I + L_i^T C_ii L_i) over state 0 (ties: the lowest index) and conditions on it: M = I + L*^T C** L*
// = G G^T, B_i,t = C_i*(t) L* G^-T with C_i*(t) = C_i*(0) - sum_{s<t} B_i,s B_*,s^T, C_ii -= B_i,t B_i,t^T. Per candidate
// in HBM: Ja Jb, L, C_ii(t), the history B_i,0..t (kk D^2), gain, d2 and the state (the SPG_CAND_* value it reports).
struct SelArgs {
    const double *arena;
    const int64_t *vpo;
    const int32_t *va, *vb, *sa, *sb;
    const double *rec;        // n x (PS + D (D + 1) / 2)
    const double *joint;      // m D x m D, row stride ld
    long long ld;
    double *J, *L, *C;        // n x 2 D^2, n x D^2, n x D^2
    double *hist;             // n x kk x D^2
    double *gain, *d2;        // n each
    int32_t *state;           // n
    double *pg;               // argmax partials: np gains, np indices
    int32_t *pi;
    int32_t *ctl;             // [0] rounds done = number selected, [1] the stop rule has fired, [2] i* of the current round
    double *pubC;             // D^2: C_**(t) as it was when i* was picked
    int32_t *sel;             // kk: the choices in order
    double *cg;               // kk: their conditional gains
    double *final_gain;       // n
    int n, kk, np;
    double min_gain, max_d2;
};
// the 2D x 2D block [[S(ra, ca), S(ra, cb)], [S(rb, ca), S(rb, cb)]] of the joint block into LDS
template <int D>
__device__ __forceinline__ void sel_load_sigma(int lane, const double *joint, long long ld, int ra, int rb, int ca, int cb, double *S) {
    constexpr int W = 2 * D;
    for (int k = lane; k < W * W; k += 64) {
        const int r = k / W, c = k - r * W;
        const int br = r < D ? ra : rb, bc = c < D ? ca : cb;
        const int rr = r < D ? r : r - D, cc = c < D ? c : c - D;
        S[k] = (br < 0 || bc < 0) ? 0.0 : joint[((long long)br * D + rr) * ld + (long long)bc * D + cc];
    }
}
// The second source of Sigma (SPG_GREEDY_LAZY, DESIGN 5g-L): no joint block. Round 0 reads the candidate's own 2D x 2D
// pair block (pslot, the blocks of sp_relative_kernel); a round reads the four blocks Sigma(a_i | b_i, a* | b*) from the
// two cache strips of the chosen candidate's endpoints. A strip is Sigma[S, v]: m D x D, row-major, strip_len = m D^2
// doubles, rows in the order of the endpoint slots sa / sb. The init and round kernels of selection and pruning are
// templates over the source (LAZY) and differ in the statement that loads Sigma alone; the joint forms get a LazyArgs
// they do not read. rank[0] = i* of the round, rank[1..L) = the next-best eligible candidates in the order of the argmax
// / argmin (-1: none), the endpoints the host may solve ahead.
struct LazyArgs {
    const double *blocks;     // per pair slot (2D)^2, row-major
    const int32_t *pslot;     // per candidate: its pair block
    const double *cache;      // the strips
    long long strip_len;
    int32_t *rank;            // L entries
    int L;
    int ca, cb;               // round kernels: the strips of a*, b* (-1: the fixed vertex)
};
// the 2D x 2D block [[S(ra, a*), S(ra, b*)], [S(rb, a*), S(rb, b*)]] out of the strips ca, cb into LDS
template <int D>
__device__ __forceinline__ void lazy_load_sigma(int lane, const double *cache, long long strip_len, int ra, int rb, int ca, int cb, double *S) {
    constexpr int W = 2 * D;
    for (int k = lane; k < W * W; k += 64) {
        const int r = k / W, c = k - r * W;
        const int br = r < D ? ra : rb, bc = c < D ? ca : cb;
        const int rr = r < D ? r : r - D, cc = c < D ? c : c - D;
        S[k] = (br < 0 || bc < 0) ? 0.0 : cache[(long long)bc * strip_len + ((long long)br * D + rr) * D + cc];
    }
}
// One wavefront per candidate, four per workgroup, the LDS slice of sp_relative_kernel: J, L, C_ii(0) = P, gain_i(0), d2
// and the state (Omega not PD: 1; max_d2 > 0 and d2 > max_d2: 2; else 0). Sigma: the candidate's own block of the joint
// covariance, or (LAZY) its pair block.
template <int D, bool LAZY>
__global__ __launch_bounds__(256) void sp_select_init_kernel(SelArgs a, LazyArgs z) {
    constexpr int W = 2 * D, DD = D * D, PS = (D == 6) ? 7 : 3, TRI = D * (D + 1) / 2, REC = PS + TRI;
    constexpr int PER = W * W + 2 * DD + D * W + 2 * DD + 2 * D;
    __shared__ double lds[4 * PER];
    __shared__ int okv[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = blockIdx.x * 4 + w;
    const bool act = i < a.n;
    double *S = lds + w * PER, *Ja = S + W * W, *Jb = Ja + DD, *T = Jb + DD, *P = T + D * W, *L = P + DD, *e = L + DD, *y = e + D;
    double *A = T, *M = T + DD;
    const double *rec = act ? a.rec + (long long)i * REC : nullptr;
    if (act) {
        if constexpr (LAZY) {
            const double *blk = z.blocks + (long long)z.pslot[i] * W * W;
            for (int k = lane; k < W * W; k += 64) S[k] = blk[k];
        } else {
            sel_load_sigma<D>(lane, a.joint, a.ld, a.sa[i], a.sb[i], a.sa[i], a.sb[i], S);
        }
        if (lane == 0) rel_geometry<D>(a.arena, a.vpo, a.va[i], a.vb[i], rec, nullptr, Ja, Jb, e);
    }
    __syncthreads();
    if (act) rel_J_sigma<D>(lane, Ja, Jb, S, T);
    __syncthreads();
    if (act && lane < DD) rel_P<D>(lane, T, Ja, Jb, P, nullptr);
    if (act && lane == 0) {
        double chi;
        okv[w] = rel_omega<D>(rec + PS, e, L, y, chi);
    }
    __syncthreads();
    const bool go = act && okv[w];
    if (go && lane < DD) rel_PL<D>(lane, P, L, A);
    __syncthreads();
    if (go && lane < DD) rel_M<D>(lane, L, A, M);
    __syncthreads();
    if (act && lane == 0) {
        double gain = __builtin_nan(""), d2 = gain;
        int st = 1;
        if (go) {
            rel_chol_M<D>(M, y, gain, d2);
            st = (a.max_d2 > 0.0 && !(d2 <= a.max_d2)) ? 2 : 0;
        }
        a.gain[i] = gain;
        a.d2[i] = d2;
        a.state[i] = st;
    }
    if (act && lane < DD) {
        a.J[(long long)i * 2 * DD + lane] = Ja[lane];
        a.J[(long long)i * 2 * DD + DD + lane] = Jb[lane];
        a.L[(long long)i * DD + lane] = L[lane];
        a.C[(long long)i * DD + lane] = P[lane];
    }
}
// (gain descending, index ascending): the order of the argmax, independent of the grid
__device__ __forceinline__ bool sel_better(double ga, int ia, double gb, int ib) { return ga > gb || (ga == gb && ia < ib); }
// the best (value, index) of a workgroup of 256 under the order `better` (sel_better / prn_better), to every thread
template <bool (*better)(double, int, double, int)>
__device__ __forceinline__ void best_reduce(double &g, int &i, double *sg, int *si) {
    const int t = threadIdx.x;
    sg[t] = g; si[t] = i;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h && better(sg[t + h], si[t + h], sg[t], si[t])) { sg[t] = sg[t + h]; si[t] = si[t + h]; }
        __syncthreads();
    }
    g = sg[0]; i = si[0];
}
// Stage 1 of the argmax (np workgroups): the best (gain, index) of the candidates in state 0 per workgroup into pg / pi.
__global__ __launch_bounds__(256) void sp_select_argmax_kernel(SelArgs a) {
    __shared__ double sg[256];
    __shared__ int si[256];
    const int stop = a.ctl[1];   // nothing in this kernel writes ctl
    double g = -__builtin_inf();
    int bi = 0x7fffffff;
    if (!stop)
        for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n; i += gridDim.x * 256)
            if (a.state[i] == 0 && sel_better(a.gain[i], i, g, bi)) { g = a.gain[i]; bi = i; }
    best_reduce<sel_better>(g, bi, sg, si);
    if (!stop && threadIdx.x == 0) { a.pg[blockIdx.x] = g; a.pi[blockIdx.x] = bi; }
}
// Stage 2 (one workgroup): the best of the partials; none, or a gain below min_gain: ctl[1] = 1. Else i* is appended to
// sel / cg, marked selected, and its C_ii is published for the round kernel. RANK (the lazy rounds) adds the ranked list:
// L - 1 passes over the candidates in state 0, each taking the best one that comes after the previous in the order of
// sel_better: no atomics, independent of the grid of stage 1.
template <int D, bool RANK>
__global__ __launch_bounds__(256) void sp_select_pick_kernel(SelArgs a, LazyArgs z) {
    constexpr int DD = D * D;
    __shared__ double sg[256];
    __shared__ int si[256];
    __shared__ int chosen;
    const int stop = a.ctl[1];   // read by every thread before the first barrier; written after it by thread 0 alone
    double g = -__builtin_inf();
    int bi = 0x7fffffff;
    if (!stop)
        for (int p = threadIdx.x; p < a.np; p += 256)
            if (sel_better(a.pg[p], a.pi[p], g, bi)) { g = a.pg[p]; bi = a.pi[p]; }
    best_reduce<sel_better>(g, bi, sg, si);
    if (stop) return;
    if (threadIdx.x == 0) {
        if (bi == 0x7fffffff || g < a.min_gain) {
            a.ctl[1] = 1;
            chosen = -1;
        } else {
            const int c = a.ctl[0];
            a.sel[c] = bi;
            a.cg[c] = g;
            a.ctl[0] = c + 1;
            a.ctl[2] = bi;
            a.state[bi] = 3;
            chosen = bi;
        }
        if constexpr (RANK) z.rank[0] = chosen;
    }
    __syncthreads();
    const int ch = chosen;
    if (ch >= 0 && threadIdx.x < DD) a.pubC[threadIdx.x] = a.C[(long long)ch * DD + threadIdx.x];
    if constexpr (RANK) {
        double pg = g;
        int pi = ch >= 0 ? bi : 0x7fffffff;
        for (int r = 1; r < z.L; r++) {
            double ng = -__builtin_inf();
            int ni = 0x7fffffff;
            if (pi != 0x7fffffff)
                for (int i = threadIdx.x; i < a.n; i += 256) {
                    if (a.state[i] != 0) continue;
                    const double gi = a.gain[i];
                    if (sel_better(pg, pi, gi, i) && sel_better(gi, i, ng, ni)) { ng = gi; ni = i; }
                }
            __syncthreads();   // every thread has read sg[0] / si[0] of the previous reduction
            best_reduce<sel_better>(ng, ni, sg, si);
            if (threadIdx.x == 0) z.rank[r] = ni == 0x7fffffff ? -1 : ni;
            pg = ng; pi = ni;
        }
    }
}
// Conditions every candidate still in state 0, and i* itself, on i* (read from ctl). One wavefront per candidate. Sigma:
// the block (a_i | b_i, a* | b*) of the joint covariance, or (LAZY) of the strips z.ca, z.cb.
template <int D, bool LAZY>
__global__ __launch_bounds__(256) void sp_select_round_kernel(SelArgs a, LazyArgs z) {
    constexpr int W = 2 * D, DD = D * D;
    constexpr int PER = W * W + 4 * DD + D * W + 8 * DD + D;
    __shared__ double lds[4 * PER];
    if (a.ctl[1]) return;   // nothing in this kernel writes ctl
    const int s = a.ctl[2], t = a.ctl[0] - 1;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = blockIdx.x * 4 + w;
    const bool act = i < a.n && (i == s || a.state[i] == 0), go = act && i != s;
    double *S = lds + w * PER, *Ji = S + W * W, *Js = Ji + 2 * DD, *T = Js + 2 * DD, *X = T + D * W, *Ls = X + DD, *Ms = Ls + DD, *As = Ms + DD,
           *K = As + DD, *B = K + DD, *Li = B + DD, *Ci = Li + DD, *y = Ci + DD;
    if (act) {
        if constexpr (LAZY) lazy_load_sigma<D>(lane, z.cache, z.strip_len, a.sa[i], a.sb[i], z.ca, z.cb, S);
        else sel_load_sigma<D>(lane, a.joint, a.ld, a.sa[i], a.sb[i], a.sa[s], a.sb[s], S);
        for (int k = lane; k < 2 * DD; k += 64) {
            Ji[k] = a.J[(long long)i * 2 * DD + k];
            Js[k] = a.J[(long long)s * 2 * DD + k];
        }
        if (lane < DD) {
            Ls[lane] = a.L[(long long)s * DD + lane];
            Ms[lane] = a.pubC[lane];
            Li[lane] = a.L[(long long)i * DD + lane];
            Ci[lane] = a.C[(long long)i * DD + lane];
        }
        if (lane < D) y[lane] = 0.0;
    }
    __syncthreads();
    if (act) {
        rel_J_sigma<D>(lane, Ji, Ji + DD, S, T);
        if (lane < DD) rel_PL<D>(lane, Ms, Ls, As);   // C** L*
    }
    __syncthreads();
    if (act && lane < DD) {
        rel_M<D>(lane, Ls, As, Ms);                    // M = I + L*^T C** L*
        const int r = lane / D, c = lane - r * D;      // X = C_i*(t), every (r, c): it is not symmetric
        double x = 0;
        for (int q = 0; q < D; q++) x += T[r * W + q] * Js[c * D + q];
        for (int q = 0; q < D; q++) x += T[r * W + D + q] * Js[DD + c * D + q];
        const double *hi = a.hist + (long long)i * a.kk * DD + r * D, *hs = a.hist + (long long)s * a.kk * DD + c * D;
        for (int u = 0; u < t; u++, hi += DD, hs += DD) {
            double d = 0;
            for (int q = 0; q < D; q++) d += hi[q] * hs[q];
            x -= d;
        }
        X[lane] = x;
    }
    __syncthreads();
    if (act && lane == 0) {
        double g, d2;
        rel_chol_M<D>(Ms, y, g, d2);                   // G in the lower triangle of Ms
    }
    __syncthreads();
    if (act && lane < D) {                             // K = L* G^-T, row `lane`: K G^T = L*
        const int r = lane;
        for (int j = 0; j < D; j++) {
            double v = (j <= r) ? Ls[r * D + j] : 0.0;
            for (int q = 0; q < j; q++) v -= K[r * D + q] * Ms[j * D + q];
            K[r * D + j] = v / Ms[j * D + j];
        }
    }
    __syncthreads();
    if (act && lane < DD) {                            // B_i,t = X K, appended to the history
        const int r = lane / D, c = lane - r * D;
        double v = 0;
        for (int q = 0; q < D; q++) v += X[r * D + q] * K[q * D + c];
        B[lane] = v;
        a.hist[((long long)i * a.kk + t) * DD + lane] = v;
    }
    __syncthreads();
    if (act && lane < DD) {                            // C_ii -= B B^T, r <= c, mirrored
        const int r = lane / D, c = lane - r * D;
        if (r <= c) {
            double d = 0;
            for (int q = 0; q < D; q++) d += B[r * D + q] * B[c * D + q];
            const double v = Ci[r * D + c] - d;
            Ci[r * D + c] = v;
            Ci[c * D + r] = v;
        }
    }
    __syncthreads();
    if (act && lane < DD) {
        a.C[(long long)i * DD + lane] = Ci[lane];
        if (go) rel_PL<D>(lane, Ci, Li, As);
    }
    __syncthreads();
    if (go && lane < DD) rel_M<D>(lane, Li, As, Ms);
    __syncthreads();
    if (go && lane == 0) {
        double g, d2;
        rel_chol_M<D>(Ms, y, g, d2);
        a.gain[i] = g;
    }
}
// final_gain: the conditional gain after the last round of every candidate still in state 0, NaN for the others
__global__ __launch_bounds__(256) void sp_select_gather_kernel(SelArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) a.final_gain[i] = a.state[i] == 0 ? a.gain[i] : __builtin_nan("");
}

// Greedy pruning of the graph's own binary edges by conditional information loss (spg_graph_prune_candidates, DESIGN
// 5g-P): the recurrence of the selection above with the sign turned. Candidate i is live edge eidx[i] of the staged graph
// (its record is read from the arena, its endpoints from the staged edge list); with C_ij as above, round t takes i* =
// argmin of loss_i = -1/2 ln det M_i, M_i = I - L_i^T C_ii L_i = G G^T, over the candidates in state 0 whose smallest
// squared pivot (the margin) is >= min_margin, and conditions on its removal: B_i,t = C_i*(t) L* G^-T with C_i*(t) =
// C_i*(0) + sum_{s<t} B_i,s B_*,s^T, C_ii += B_i,t B_i,t^T. States: 0 live, 1 Omega not PD, 3 pruned.
// The same kernels, instantiated with OBJ_STAT, are the greedy data snooping of spg_graph_detect_outliers (DESIGN 5g-O):
// the objective is stat_i = |G^-1 L_i^T e_i|^2 instead of the loss (kept in `loss`), i* is its argmax, the stop rule is
// min_stat, and a round also moves the residuals, e_i += B_i,t w with w = G^-1 L*^T e*. Everything that differs sits
// under `if constexpr (OBJ == OBJ_STAT)`. The two fields only one objective reads share their place with the other's, so
// that the argument block, and with it the code of the OBJ_LOSS instantiations, is what it was before OBJ existed.
enum { OBJ_LOSS = 0, OBJ_STAT = 1 };
struct PruneArgs {
    const double *arena;
    const int64_t *vpo;
    const spg_edge_ref *er;   // the staged live edges
    const int32_t *ev;
    const int32_t *eidx, *sa, *sb;
    const double *joint;      // m D x m D, row stride ld
    long long ld;
    double *J, *L, *C;        // n x 2 D^2, n x D^2, n x D^2
    double *hist;             // n x kk x D^2
    double *loss, *margin;    // n each: of the current round
    double *tr0;              // n: tr(L_i^T C_ii(0) L_i), the trace term of the KLD
    int32_t *state;           // n
    double *pg;               // argmin partials: np losses, np indices
    int32_t *pi;
    int32_t *ctl;             // [0] rounds done = number pruned, [1] a stop rule has fired, [2] i* of the current round
    double *pubC;             // D^2: C_**(t) as it was when i* was picked
    union {
        double *kldsum;       // OBJ_LOSS: one double, the cumulative KLD (written by thread 0 of argmin stage 2 alone)
        double *e;            // OBJ_STAT: n x D, e_i(t); pubC is then D^2 + D long, e* behind C**
    };
    int32_t *sel;             // kk: the choices in order
    double *cl, *ck;          // kk: their conditional losses, the cumulative KLD after each
    double *final_loss, *final_margin;   // n each
    int32_t *status;          // n: SPG_PRUNE_*
    int n, kk, np;
    union {
        double max_loss;      // OBJ_LOSS
        double min_stat;      // OBJ_STAT
    };
    double max_kld, min_margin;
};
// lanes < D^2: M = I - L^T A, r <= c, mirrored
template <int D>
__device__ __forceinline__ void rel_M_down(int lane, const double *L, const double *A, double *M) {
    const int r = lane / D, c = lane - r * D;
    if (r <= c) {
        double s = (r == c) ? 1.0 : 0.0;
        for (int t = r; t < D; t++) s -= L[t * D + r] * A[t * D + c];
        M[r * D + c] = s;
        M[c * D + r] = s;
    }
}
// lane 0: M = G G^T in place (lower triangle), checked: stops at the first squared pivot that is not finite, <= 0 or below
// min_margin (false; loss = NaN). margin = the smallest squared pivot seen (NaN for a pivot that is not finite), loss =
// -sum log G_jj = -1/2 ln det M.
template <int D>
__device__ __forceinline__ bool rel_chol_downdate(double *M, double min_margin, double &loss_out, double &margin_out) {
    double loss = 0, margin = __builtin_inf();
    bool ok = true;
    for (int j = 0; j < D; j++) {
        double d = M[j * D + j];
        for (int k = 0; k < j; k++) d -= M[j * D + k] * M[j * D + k];
        if (!isfinite(d)) { margin = __builtin_nan(""); ok = false; break; }
        margin = d < margin ? d : margin;
        if (!(d > 0.0) || d < min_margin) { ok = false; break; }
        d = sqrt(d);
        M[j * D + j] = d;
        loss -= log(d);
        for (int r = j + 1; r < D; r++) {
            double v = M[r * D + j];
            for (int k = 0; k < j; k++) v -= M[r * D + k] * M[j * D + k];
            M[r * D + j] = v / d;
        }
    }
    loss_out = ok ? loss : __builtin_nan("");
    margin_out = margin;
    return ok;
}
// lane 0: y = L^T e (L lower triangular), then G x = y in place (G: the lower triangle of M); returns |x|^2
template <int D>
__device__ __forceinline__ double rel_whiten_solve(const double *L, const double *e, const double *G, double *y) {
    for (int c = 0; c < D; c++) {
        double s = 0;
        for (int r = c; r < D; r++) s += L[r * D + c] * e[r];
        y[c] = s;
    }
    double n2 = 0;
    for (int j = 0; j < D; j++) {
        double x = y[j];
        for (int k = 0; k < j; k++) x -= G[j * D + k] * y[k];
        x /= G[j * D + j];
        y[j] = x;
        n2 += x * x;
    }
    return n2;
}
// One wavefront per candidate, four per workgroup, the LDS slice of sp_select_init_kernel: J, L, C_ii(0) = P, tr0, the
// loss (OBJ_STAT: the statistic, and e_i(0)) and the margin of round 0, and the state (Omega not finite or not PD: 1,
// else 0). Sigma: as there.
template <int D, bool LAZY, int OBJ>
__global__ __launch_bounds__(256) void sp_prune_init_kernel(PruneArgs a, LazyArgs z) {
    constexpr int W = 2 * D, DD = D * D, PS = (D == 6) ? 7 : 3;
    constexpr int PER = W * W + 2 * DD + D * W + 2 * DD + 2 * D;
    __shared__ double lds[4 * PER];
    __shared__ int okv[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = blockIdx.x * 4 + w;
    const bool act = i < a.n;
    double *S = lds + w * PER, *Ja = S + W * W, *Jb = Ja + DD, *T = Jb + DD, *P = T + D * W, *L = P + DD, *e = L + DD, *y = e + D;
    double *A = T, *M = T + DD;
    const spg_edge_ref *er = act ? a.er + a.eidx[i] : nullptr;
    const double *rec = act ? a.arena + er->off : nullptr;
    if (act) {
        if constexpr (LAZY) {
            const double *blk = z.blocks + (long long)z.pslot[i] * W * W;
            for (int k = lane; k < W * W; k += 64) S[k] = blk[k];
        } else {
            sel_load_sigma<D>(lane, a.joint, a.ld, a.sa[i], a.sb[i], a.sa[i], a.sb[i], S);
        }
        if (lane == 0) rel_geometry<D>(a.arena, a.vpo, a.ev[er->vbegin], a.ev[er->vbegin + 1], rec, nullptr, Ja, Jb, e);
    }
    __syncthreads();
    if (act) rel_J_sigma<D>(lane, Ja, Jb, S, T);
    __syncthreads();
    if (act && lane < DD) rel_P<D>(lane, T, Ja, Jb, P, nullptr);
    if (act && lane == 0) {
        double chi;
        okv[w] = rel_omega<D>(rec + PS, e, L, y, chi);
    }
    __syncthreads();
    const bool go = act && okv[w];
    if (go && lane < DD) rel_PL<D>(lane, P, L, A);
    __syncthreads();
    if (go && lane == 0) {           // tr(L^T P L) before M takes A's neighbour
        double tr = 0;
        for (int c = 0; c < D; c++)
            for (int t = c; t < D; t++) tr += L[t * D + c] * A[t * D + c];
        a.tr0[i] = tr;
    }
    if (go && lane < DD) rel_M_down<D>(lane, L, A, M);
    __syncthreads();
    if (act && lane == 0) {
        double loss = __builtin_nan(""), margin = loss;
        if (go) {
            const bool ok = rel_chol_downdate<D>(M, a.min_margin, loss, margin);
            if constexpr (OBJ == OBJ_STAT) {
                if (ok) loss = rel_whiten_solve<D>(L, e, M, y);
            }
        } else {
            a.tr0[i] = loss;
        }
        a.loss[i] = loss;
        a.margin[i] = margin;
        a.state[i] = go ? 0 : 1;
    }
    if (act && lane < DD) {
        a.J[(long long)i * 2 * DD + lane] = Ja[lane];
        a.J[(long long)i * 2 * DD + DD + lane] = Jb[lane];
        a.L[(long long)i * DD + lane] = L[lane];
        a.C[(long long)i * DD + lane] = P[lane];
    }
    if constexpr (OBJ == OBJ_STAT) {
        if (act && lane < D) a.e[(long long)i * D + lane] = e[lane];   // written by lane 0 three barriers ago
    }
}
// (loss ascending, index ascending): the order of the argmin, independent of the grid
__device__ __forceinline__ bool prn_better(double ga, int ia, double gb, int ib) { return ga < gb || (ga == gb && ia < ib); }
// (statistic descending, index ascending): the order of the outlier argmax
__device__ __forceinline__ bool out_better(double ga, int ia, double gb, int ib) { return ga > gb || (ga == gb && ia < ib); }
// the order of an objective, and the value every candidate beats
template <int OBJ>
__device__ __forceinline__ bool obj_better(double ga, int ia, double gb, int ib) {
    if constexpr (OBJ == OBJ_STAT) return out_better(ga, ia, gb, ib);
    else return prn_better(ga, ia, gb, ib);
}
template <int OBJ>
__device__ __forceinline__ double obj_worst() { return OBJ == OBJ_STAT ? -__builtin_inf() : __builtin_inf(); }
// Stage 1 of the argmin (np workgroups): the best (loss, index) per workgroup of the candidates in state 0 that are
// eligible this round (a loss that is not NaN, margin >= min_margin; the others stay in state 0) into pg / pi.
template <int OBJ>
__global__ __launch_bounds__(256) void sp_prune_argmin_kernel(PruneArgs a) {
    __shared__ double sg[256];
    __shared__ int si[256];
    const int stop = a.ctl[1];   // nothing in this kernel writes ctl
    double g = obj_worst<OBJ>();
    int bi = 0x7fffffff;
    if (!stop)
        for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n; i += gridDim.x * 256) {
            const double l = a.loss[i];
            if (a.state[i] == 0 && l == l && a.margin[i] >= a.min_margin && obj_better<OBJ>(l, i, g, bi)) { g = l; bi = i; }
        }
    best_reduce<obj_better<OBJ>>(g, bi, sg, si);
    if (!stop && threadIdx.x == 0) { a.pg[blockIdx.x] = g; a.pi[blockIdx.x] = bi; }
}
// Stage 2 (one workgroup): the best of the partials; none, a loss above max_loss or a cumulative KLD above max_kld:
// ctl[1] = 1. Else i* is appended to sel / cl / ck, marked pruned, and its C_ii is published for the round kernel. RANK
// (the lazy rounds) adds the ranked list over the candidates eligible this round, in the order of the objective.
// OBJ_STAT: the one stop rule is a best statistic below min_stat, there is no KLD, and e* is published behind C**.
template <int D, bool RANK, int OBJ>
__global__ __launch_bounds__(256) void sp_prune_pick_kernel(PruneArgs a, LazyArgs z) {
    constexpr int DD = D * D;
    __shared__ double sg[256];
    __shared__ int si[256];
    __shared__ int chosen;
    const int stop = a.ctl[1];   // read by every thread before the first barrier; written after it by thread 0 alone
    double g = obj_worst<OBJ>();
    int bi = 0x7fffffff;
    if (!stop)
        for (int p = threadIdx.x; p < a.np; p += 256)
            if (obj_better<OBJ>(a.pg[p], a.pi[p], g, bi)) { g = a.pg[p]; bi = a.pi[p]; }
    best_reduce<obj_better<OBJ>>(g, bi, sg, si);
    if (stop) return;
    if (threadIdx.x == 0) {
        chosen = -1;
        if constexpr (OBJ == OBJ_STAT) {
            if (bi == 0x7fffffff || (a.min_stat > 0.0 && g < a.min_stat)) {
                a.ctl[1] = 1;
            } else {
                const int c = a.ctl[0];
                a.sel[c] = bi;
                a.cl[c] = g;
                a.ctl[0] = c + 1;
                a.ctl[2] = bi;
                a.state[bi] = 3;
                chosen = bi;
            }
        } else if (bi == 0x7fffffff || (a.max_loss > 0.0 && g > a.max_loss)) {
            a.ctl[1] = 1;
        } else {
            const double kld = a.kldsum[0] + (g - 0.5 * a.tr0[bi]);
            if (a.max_kld > 0.0 && kld > a.max_kld) {
                a.ctl[1] = 1;
            } else {
                const int c = a.ctl[0];
                a.sel[c] = bi;
                a.cl[c] = g;
                a.ck[c] = kld;
                a.kldsum[0] = kld;
                a.ctl[0] = c + 1;
                a.ctl[2] = bi;
                a.state[bi] = 3;
                chosen = bi;
            }
        }
        if constexpr (RANK) z.rank[0] = chosen;
    }
    __syncthreads();
    const int ch = chosen;
    if (ch >= 0 && threadIdx.x < DD) a.pubC[threadIdx.x] = a.C[(long long)ch * DD + threadIdx.x];
    if constexpr (OBJ == OBJ_STAT) {
        if (ch >= 0 && threadIdx.x < D) a.pubC[DD + threadIdx.x] = a.e[(long long)ch * D + threadIdx.x];
    }
    if constexpr (RANK) {
        double pg = g;
        int pi = ch >= 0 ? bi : 0x7fffffff;
        for (int r = 1; r < z.L; r++) {
            double ng = obj_worst<OBJ>();
            int ni = 0x7fffffff;
            if (pi != 0x7fffffff)
                for (int i = threadIdx.x; i < a.n; i += 256) {
                    const double l = a.loss[i];
                    if (a.state[i] != 0 || !(l == l) || !(a.margin[i] >= a.min_margin)) continue;
                    if (obj_better<OBJ>(pg, pi, l, i) && obj_better<OBJ>(l, i, ng, ni)) { ng = l; ni = i; }
                }
            __syncthreads();   // every thread has read sg[0] / si[0] of the previous reduction
            best_reduce<obj_better<OBJ>>(ng, ni, sg, si);
            if (threadIdx.x == 0) z.rank[r] = ni == 0x7fffffff ? -1 : ni;
            pg = ng; pi = ni;
        }
    }
}
// Conditions every candidate still in state 0, and i* itself, on the removal of i* (read from ctl), then re-evaluates the
// candidate's own M, loss and margin. One wavefront per candidate. M of i* passed the margin test when it was picked; if
// its factorisation fails all the same, the candidate gets a NaN loss and margin and nothing else of it is touched.
// Sigma: as in sp_select_round_kernel. OBJ_STAT: the slice grows by e*, w = G^-1 L*^T e*, e_i and the solve's vector
// (4 D doubles: 678 per wavefront at D = 6, 21.7 KB per workgroup); e_i += B_i,t w, and the objective is the statistic.
template <int D, bool LAZY, int OBJ>
__global__ __launch_bounds__(256) void sp_prune_round_kernel(PruneArgs a, LazyArgs z) {
    constexpr int W = 2 * D, DD = D * D;
    constexpr int PER = W * W + 4 * DD + D * W + 8 * DD + D + (OBJ == OBJ_STAT ? 4 * D : 0);
    __shared__ double lds[4 * PER];
    __shared__ int okv[4];
    if (a.ctl[1]) return;   // nothing in this kernel writes ctl
    const int s = a.ctl[2], t = a.ctl[0] - 1;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = blockIdx.x * 4 + w;
    const bool act = i < a.n && (i == s || a.state[i] == 0), go = act && i != s;
    double *S = lds + w * PER, *Ji = S + W * W, *Js = Ji + 2 * DD, *T = Js + 2 * DD, *X = T + D * W, *Ls = X + DD, *Ms = Ls + DD, *As = Ms + DD,
           *K = As + DD, *B = K + DD, *Li = B + DD, *Ci = Li + DD;
    double *es = Ci + DD + D, *wv = es + D, *ei = wv + D, *yi = ei + D;   // OBJ_STAT only: behind the slice of OBJ_LOSS
    if (act) {
        if constexpr (LAZY) lazy_load_sigma<D>(lane, z.cache, z.strip_len, a.sa[i], a.sb[i], z.ca, z.cb, S);
        else sel_load_sigma<D>(lane, a.joint, a.ld, a.sa[i], a.sb[i], a.sa[s], a.sb[s], S);
        for (int k = lane; k < 2 * DD; k += 64) {
            Ji[k] = a.J[(long long)i * 2 * DD + k];
            Js[k] = a.J[(long long)s * 2 * DD + k];
        }
        if (lane < DD) {
            Ls[lane] = a.L[(long long)s * DD + lane];
            Ms[lane] = a.pubC[lane];
            Li[lane] = a.L[(long long)i * DD + lane];
            Ci[lane] = a.C[(long long)i * DD + lane];
        }
        if constexpr (OBJ == OBJ_STAT) {
            if (lane < D) {
                es[lane] = a.pubC[DD + lane];
                ei[lane] = a.e[(long long)i * D + lane];
            }
        }
    }
    __syncthreads();
    if (act) {
        rel_J_sigma<D>(lane, Ji, Ji + DD, S, T);
        if (lane < DD) rel_PL<D>(lane, Ms, Ls, As);   // C** L*
    }
    __syncthreads();
    if (act && lane < DD) {
        rel_M_down<D>(lane, Ls, As, Ms);               // M = I - L*^T C** L*
        const int r = lane / D, c = lane - r * D;      // X = C_i*(t), every (r, c): it is not symmetric
        double x = 0;
        for (int q = 0; q < D; q++) x += T[r * W + q] * Js[c * D + q];
        for (int q = 0; q < D; q++) x += T[r * W + D + q] * Js[DD + c * D + q];
        const double *hi = a.hist + (long long)i * a.kk * DD + r * D, *hs = a.hist + (long long)s * a.kk * DD + c * D;
        for (int u = 0; u < t; u++, hi += DD, hs += DD) {
            double d = 0;
            for (int q = 0; q < D; q++) d += hi[q] * hs[q];
            x += d;
        }
        X[lane] = x;
    }
    __syncthreads();
    if (act && lane == 0) {
        double l, m;
        okv[w] = rel_chol_downdate<D>(Ms, 0.0, l, m);  // G in the lower triangle of Ms
        if (!okv[w]) { a.loss[i] = __builtin_nan(""); a.margin[i] = __builtin_nan(""); }
        if constexpr (OBJ == OBJ_STAT) {
            if (okv[w]) rel_whiten_solve<D>(Ls, es, Ms, wv);   // w = G^-1 L*^T e*
        }
    }
    __syncthreads();
    const bool upd = act && okv[w];
    if (upd && lane < D) {                             // K = L* G^-T, row `lane`: K G^T = L*
        const int r = lane;
        for (int j = 0; j < D; j++) {
            double v = (j <= r) ? Ls[r * D + j] : 0.0;
            for (int q = 0; q < j; q++) v -= K[r * D + q] * Ms[j * D + q];
            K[r * D + j] = v / Ms[j * D + j];
        }
    }
    __syncthreads();
    if (upd && lane < DD) {                            // B_i,t = X K, appended to the history
        const int r = lane / D, c = lane - r * D;
        double v = 0;
        for (int q = 0; q < D; q++) v += X[r * D + q] * K[q * D + c];
        B[lane] = v;
        a.hist[((long long)i * a.kk + t) * DD + lane] = v;
    }
    __syncthreads();
    if (upd && lane < DD) {                            // C_ii += B B^T, r <= c, mirrored
        const int r = lane / D, c = lane - r * D;
        if (r <= c) {
            double d = 0;
            for (int q = 0; q < D; q++) d += B[r * D + q] * B[c * D + q];
            const double v = Ci[r * D + c] + d;
            Ci[r * D + c] = v;
            Ci[c * D + r] = v;
        }
    }
    if constexpr (OBJ == OBJ_STAT) {
        if (upd && go && lane < D) {                   // e_i += B_i,t w
            double v = ei[lane];
            for (int q = 0; q < D; q++) v += B[lane * D + q] * wv[q];
            ei[lane] = v;
            a.e[(long long)i * D + lane] = v;
        }
    }
    __syncthreads();
    const bool re = upd && go;
    if (upd && lane < DD) {
        a.C[(long long)i * DD + lane] = Ci[lane];
        if (go) rel_PL<D>(lane, Ci, Li, As);
    }
    __syncthreads();
    if (re && lane < DD) rel_M_down<D>(lane, Li, As, Ms);
    __syncthreads();
    if (re && lane == 0) {
        double l, m;
        const bool ok = rel_chol_downdate<D>(Ms, a.min_margin, l, m);
        if constexpr (OBJ == OBJ_STAT) {
            if (ok) l = rel_whiten_solve<D>(Li, ei, Ms, yi);
        } else {
            (void)ok;
        }
        a.loss[i] = l;
        a.margin[i] = m;
    }
}
// final_loss / final_margin / status after the last round: a candidate still in state 0 is SPG_PRUNE_BRIDGE when its
// margin is below min_margin or NaN (final_loss NaN), else SPG_PRUNE_KEPT. The SPG_OUTLIER_* values are the same four, and
// `loss` then holds the statistic.
__global__ __launch_bounds__(256) void sp_prune_gather_kernel(PruneArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const double nan = __builtin_nan("");
    const int st = a.state[i];
    const double l = a.loss[i], m = a.margin[i];
    const bool kept = st == 0 && l == l && m >= a.min_margin;
    a.final_loss[i] = kept ? l : nan;
    a.final_margin[i] = st == 0 ? m : nan;
    a.status[i] = st != 0 ? st : kept ? 0 : 2;
}

// Fills the strips of LazyArgs: cache[strip[c]][(j D + r) D + cc] = ws[srow[j] + r R + D c + cc], the solved panel rows
// of every endpoint vertex j (srow: where its first row starts in the panel workspace) into the strips of the panel's
// ncol column vertices. One thread per element, the D ncol panel columns fastest; every strip element has one writer.
__global__ __launch_bounds__(256) void sp_strip_rows_kernel(const double *ws, const int64_t *srow, int m, int D, int R, const int32_t *strip, int ncol,
                                                             long long strip_len, double *cache) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, per = (long long)D * ncol;
    if (idx >= (long long)m * D * per) return;
    const long long row = idx / per;
    const int e = (int)(idx - row * per), c = e / D, cc = e - c * D;
    const int j = (int)(row / D), r = (int)(row - (long long)j * D);
    cache[(long long)strip[c] * strip_len + row * D + cc] = ws[srow[j] + (long long)r * R + e];
}

// Per-vertex KLD of two D x D marginals, kullbackLeiblerDivergence(diff, Sx^-1, Sy^-1, InformationInformation)
// (src/utils.cpp:70-97) = 0.5 (tr(Sx^-1 Sy) + diff^T Sx^-1 diff + log det Sx - log det Sy - D), through the Cholesky
// factors Sx = Lx Lx^T, Sy = Ly Ly^T: tr = || Lx^-1 Ly ||_F^2, Mahalanobis = || Lx^-1 diff ||^2. One lane per vertex,
// fp64 in registers. bad[0] / bad[1]: Sy / Sx not positive definite.
template <int D>
__global__ __launch_bounds__(64) void sp_marginal_kld_kernel(const double *sx, const double *sy, const double *diff, int n, double *kld, int *bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double Lx[D][D], Ly[D][D];
#pragma unroll
    for (int r = 0; r < D; r++)
#pragma unroll
        for (int c = 0; c < D; c++) { Lx[r][c] = sx[(long long)i * D * D + r * D + c]; Ly[r][c] = sy[(long long)i * D * D + r * D + c]; }
    bool okx = true, oky = true;
    double ldx = 0, ldy = 0;
#pragma unroll
    for (int j = 0; j < D; j++) {
#pragma unroll
        for (int k = 0; k < j; k++) { Lx[j][j] -= Lx[j][k] * Lx[j][k]; Ly[j][j] -= Ly[j][k] * Ly[j][k]; }
        okx = okx && Lx[j][j] > 0.0 && isfinite(Lx[j][j]);
        oky = oky && Ly[j][j] > 0.0 && isfinite(Ly[j][j]);
        Lx[j][j] = sqrt(Lx[j][j]);
        Ly[j][j] = sqrt(Ly[j][j]);
        ldx += log(Lx[j][j]);
        ldy += log(Ly[j][j]);
#pragma unroll
        for (int r = j + 1; r < D; r++) {
#pragma unroll
            for (int k = 0; k < j; k++) { Lx[r][j] -= Lx[r][k] * Lx[j][k]; Ly[r][j] -= Ly[r][k] * Ly[j][k]; }
            Lx[r][j] /= Lx[j][j];
            Ly[r][j] /= Ly[j][j];
        }
    }
    if (!okx || !oky) {
        if (!oky) bad[0] = 1;
        if (!okx) bad[1] = 1;
        kld[i] = __builtin_nan("");
        return;
    }
    double tr = 0, mahal = 0, z[D];
#pragma unroll
    for (int c = 0; c <= D; c++) {     // columns of Ly, then diff
#pragma unroll
        for (int r = 0; r < D; r++) {
            double s = (c == D) ? diff[(long long)i * D + r] : (r >= c ? Ly[r][c] : 0.0);
#pragma unroll
            for (int k = 0; k < r; k++) s -= Lx[r][k] * z[k];
            z[r] = s / Lx[r][r];
            if (c == D) mahal += z[r] * z[r]; else tr += z[r] * z[r];
        }
    }
    kld[i] = 0.5 * (tr + mahal + 2 * ldx - 2 * ldy - D);
}

// ------------------------------------------------------------------------------------------ host side
struct SpStep {
    enum Kind { GEMM, DIAG, EXTADD, GATHER } kind;
    int64_t begin;
    int32_t count, ymax;
};

struct SparseSolver {
    Plan plan;
    int D = 0;
    DevBuf pool, linv, work, zpool, partial, ibuf, lbuf, gemm_items, diag_items, pairs, kept_list, own_bad;
    SpDev dev{};
    std::vector<SpStep> fact_steps, sel_steps;
    std::vector<int64_t> zoff;
    int64_t zpool_len = 0;
    int n_kept_sn = 0;
    double selinv_flops = 0;   // of the selected inverse's tile products as executed (pads included)
    const int64_t *d_zoff = nullptr;
    size_t bytes = 0;

    static int up(DevBuf &b, const void *src, size_t bytes_) {
        if (hipMalloc(&b.p, std::max<size_t>(bytes_, 8)) != hipSuccess) return SPG_ENOMEM;
        if (bytes_ && hipMemcpy(b.p, src, bytes_, hipMemcpyHostToDevice) != hipSuccess) return SPG_EHIP;
        return 0;
    }

    // with_selinv: also the item lists of the selected inverse over the kept supernodes (index >= n_marg_sn)
    int init(Plan &&p, bool with_selinv, char *err, size_t errlen) {
        plan = std::move(p);
        const Plan &P = plan;
        D = P.D;
        const int nsn = P.nsn;
        for (int32_t r : P.rel) if (r < 0) { snprintf(err, errlen, "sparse plan: a child's boundary row is missing in its parent"); return SPG_ESTATE; }
        zoff.assign((size_t)nsn, 0);
        if (with_selinv) for (int s = P.n_marg_sn; s < nsn; s++) { zoff[s] = zpool_len; zpool_len += (int64_t)P.NP[s] * P.NP[s]; }
        bytes = (size_t)(P.pool + P.linv_pool + P.work + zpool_len) * 8;
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        if (bytes + (1ull << 30) > free_b) {
            snprintf(err, errlen, "sparse factorisation needs %.1f GB of fronts (%d supernodes), %.1f GB are free", bytes * 1e-9, nsn, free_b * 1e-9);
            return SPG_ECAPACITY;
        }
        if (hipMalloc(&pool.p, std::max<int64_t>(P.pool, 1) * 8) != hipSuccess || hipMalloc(&linv.p, std::max<int64_t>(P.linv_pool, 1) * 8) != hipSuccess ||
            hipMalloc(&work.p, std::max<int64_t>(P.work, 1) * 8) != hipSuccess || hipMalloc(&zpool.p, std::max<int64_t>(zpool_len, 1) * 8) != hipSuccess ||
            hipMalloc(&partial.p, (size_t)std::max(nsn, 1) * 8) != hipSuccess || hipMalloc(&own_bad.p, 8) != hipSuccess) {
            snprintf(err, errlen, "hipMalloc of the fronts failed (%.1f GB)", bytes * 1e-9);
            return SPG_ENOMEM;
        }
        // structure arrays: one int32 buffer, one int64 buffer
        std::vector<int32_t> ib;
        auto put = [&](const std::vector<int32_t> &v) { size_t o = ib.size(); ib.insert(ib.end(), v.begin(), v.end()); if (v.empty()) ib.push_back(0); return o; };
        const size_t o_first = put(P.first), o_rowptr = put(P.rowptr), o_rows = put(P.rows), o_rel = put(P.rel), o_cp = put(P.childptr),
                     o_child = put(P.child), o_np = put(P.NP), o_nb = put(P.NB), o_snof = put(P.sn_of), o_lsn = put(P.level_sn);
        std::vector<int64_t> lb;
        lb.insert(lb.end(), P.foff.begin(), P.foff.end());
        lb.insert(lb.end(), P.loff.begin(), P.loff.end());
        lb.insert(lb.end(), P.woff.begin(), P.woff.end());
        lb.insert(lb.end(), zoff.begin(), zoff.end());
        int rc;
        if ((rc = up(ibuf, ib.data(), ib.size() * 4)) || (rc = up(lbuf, lb.data(), lb.size() * 8))) return rc;
        const int32_t *I = (const int32_t *)ibuf.p;
        const int64_t *L = (const int64_t *)lbuf.p;
        dev = SpDev{(double *)pool.p, (double *)linv.p, (double *)work.p, I + o_first, I + o_rowptr, I + o_rows, I + o_rel, I + o_cp, I + o_child,
                    I + o_np, I + o_nb, I + o_snof, I + o_lsn, L, L + nsn, L + 2 * (size_t)nsn, D, nsn};
        d_zoff = L + 3 * (size_t)nsn;
        build_items(with_selinv);
        return upload_items(err, errlen);
    }

    std::vector<GemmItem> h_gemm;
    std::vector<DiagItem> h_diag;
    std::vector<EaPair> h_pairs;

    double *front(int s) const { return (double *)pool.p + plan.foff[s]; }
    double *ztile(int s) const { return (double *)zpool.p + zoff[s]; }

    void gemm(std::vector<SpStep> &steps, size_t begin) {
        if (h_gemm.size() > begin) steps.push_back({SpStep::GEMM, (int64_t)begin, (int32_t)(h_gemm.size() - begin), 0});
    }

    void build_items(bool with_selinv) {
        const Plan &P = plan;
        const int32_t *d_rel = dev.rel;
        for (int l = 0; l < P.nlevels; l++) {
            const int32_t *sn = P.level_sn.data() + P.level_ptr[l];
            const int cnt = P.level_ptr[l + 1] - P.level_ptr[l];
            // extend-add, one launch per child rank
            for (int k = 0;; k++) {
                const size_t b0 = h_pairs.size();
                int ymax = 0;
                for (int i = 0; i < cnt; i++) {
                    const int s = sn[i];
                    if (P.childptr[s + 1] - P.childptr[s] <= k) continue;
                    const int c = P.child[P.childptr[s] + k];
                    if (P.nrows(c) == 0) continue;
                    h_pairs.push_back({front(c) + (int64_t)P.NP[c] * P.ld(c) + P.NP[c], front(s), d_rel + P.rowptr[c], P.ld(c), P.ld(s), P.nrows(c), P.NP[s]});
                    ymax = std::max(ymax, (P.nrows(c) + 3) / 4);
                }
                if (h_pairs.size() == b0) {
                    bool more = false;
                    for (int i = 0; i < cnt && !more; i++) more = P.childptr[sn[i] + 1] - P.childptr[sn[i]] > k + 1;
                    if (!more) break;
                    continue;
                }
                fact_steps.push_back({SpStep::EXTADD, (int64_t)b0, (int32_t)(h_pairs.size() - b0), ymax});
            }
            int maxtp = 0;
            for (int i = 0; i < cnt; i++) maxtp = std::max(maxtp, P.NP[sn[i]] / 64);
            for (int p = 0; p < maxtp; p++) {
                size_t b0 = h_gemm.size();
                if (p > 0)
                    for (int i = 0; i < cnt; i++) {
                        const int s = sn[i], ld = P.ld(s), T = ld / 64;
                        if (P.NP[s] / 64 <= p) continue;
                        double *F = front(s);
                        for (int r = p; r < T; r++)
                            h_gemm.push_back({F + (int64_t)r * 64 * ld + 64 * p, F + (int64_t)r * 64 * ld, F + (int64_t)p * 64 * ld, ld, ld, ld, 64, 64, p, GI_TB | GI_ACC | GI_NEG, 0});
                    }
                gemm(fact_steps, b0);
                const size_t d0 = h_diag.size();
                for (int i = 0; i < cnt; i++) {
                    const int s = sn[i], ld = P.ld(s);
                    if (P.NP[s] / 64 <= p) continue;
                    h_diag.push_back({front(s) + (int64_t)p * 64 * (ld + 1), (double *)linv.p + P.loff[s] + (int64_t)p * 4096, ld, 0});
                }
                fact_steps.push_back({SpStep::DIAG, (int64_t)d0, (int32_t)(h_diag.size() - d0), 0});
                b0 = h_gemm.size();
                for (int i = 0; i < cnt; i++) {
                    const int s = sn[i], ld = P.ld(s), T = ld / 64;
                    if (P.NP[s] / 64 <= p) continue;
                    double *F = front(s);
                    const double *Li = (double *)linv.p + P.loff[s] + (int64_t)p * 4096;
                    for (int r = p + 1; r < T; r++) {
                        double *t = F + (int64_t)r * 64 * ld + 64 * p;
                        h_gemm.push_back({t, t, Li, ld, ld, 64, 0, 0, 1, GI_TB, 0});
                    }
                }
                gemm(fact_steps, b0);
            }
            // Schur complement of the boundary block
            const size_t b0 = h_gemm.size();
            for (int i = 0; i < cnt; i++) {
                const int s = sn[i], ld = P.ld(s), T = ld / 64, TP = P.NP[s] / 64;
                double *F = front(s);
                for (int r = TP; r < T; r++)
                    for (int c = TP; c <= r; c++)
                        h_gemm.push_back({F + (int64_t)r * 64 * ld + 64 * c, F + (int64_t)r * 64 * ld, F + (int64_t)c * 64 * ld, ld, ld, ld, 64, 64, TP, GI_TB | GI_ACC | GI_NEG, 0});
            }
            gemm(fact_steps, b0);
        }
        if (!with_selinv) return;
        const size_t sel_begin = h_gemm.size();
        // ---- selected inverse over the kept supernodes, top-down
        for (int l = P.nlevels - 1; l >= 0; l--) {
            std::vector<int> sn;
            for (int i = P.level_ptr[l]; i < P.level_ptr[l + 1]; i++) if (P.level_sn[i] >= P.n_marg_sn) sn.push_back(P.level_sn[i]);
            if (sn.empty()) continue;
            {   // Sigma_BB from the parent
                const size_t b0 = h_pairs.size();
                int ymax = 0;
                for (int s : sn) {
                    if (P.nrows(s) == 0) continue;
                    const int par = P.parent[s];
                    h_pairs.push_back({front(s) + (int64_t)P.NP[s] * P.ld(s) + P.NP[s], front(par), d_rel + P.rowptr[s], P.ld(s), P.ld(par), P.nrows(s), P.NP[par]});
                    ymax = std::max(ymax, (P.nrows(s) + 3) / 4);
                }
                if (h_pairs.size() > b0) sel_steps.push_back({SpStep::GATHER, (int64_t)b0, (int32_t)(h_pairs.size() - b0), ymax});
            }
            int maxtp = 0;
            for (int s : sn) maxtp = std::max(maxtp, P.NP[s] / 64);
            // [Z; Y] = [I; L_BS] L_SS^-1, block columns from the last to the first
            for (int st = 0; st < maxtp; st++) {
                size_t b0 = h_gemm.size();
                for (int s : sn) {
                    const int ld = P.ld(s), T = ld / 64, TP = P.NP[s] / 64, np = P.NP[s];
                    if (TP <= st) continue;
                    const int p = TP - 1 - st;
                    double *F = front(s), *Z = ztile(s);
                    const double *Lcol = F + (int64_t)(p + 1) * 64 * ld + 64 * p;    // L(p+1.., p), K stride 64 ld
                    for (int r = p + 1; r < TP; r++)      // Z(r,p) -= sum_{q=p+1..r} Z(r,q) L(q,p)
                        h_gemm.push_back({Z + (int64_t)r * 64 * np + 64 * p, Z + (int64_t)r * 64 * np + 64 * (p + 1), Lcol, np, np, ld, 64, 64 * ld, r - p, GI_ACC | GI_NEG, 0});
                    if (TP - 1 - p > 0)
                        for (int r = TP; r < T; r++)      // Y(r,p) = L(r,p) - sum_{q>p} Y(r,q) L(q,p)
                            h_gemm.push_back({F + (int64_t)r * 64 * ld + 64 * p, F + (int64_t)r * 64 * ld + 64 * (p + 1), Lcol, ld, ld, ld, 64, 64 * ld, TP - 1 - p, GI_ACC | GI_NEG, 0});
                }
                gemm(sel_steps, b0);
                b0 = h_gemm.size();
                for (int s : sn) {
                    const int ld = P.ld(s), T = ld / 64, TP = P.NP[s] / 64, np = P.NP[s];
                    if (TP <= st) continue;
                    const int p = TP - 1 - st;
                    double *F = front(s), *Z = ztile(s);
                    const double *Li = (double *)linv.p + P.loff[s] + (int64_t)p * 4096;
                    for (int r = p; r < TP; r++) { double *t = Z + (int64_t)r * 64 * np + 64 * p; h_gemm.push_back({t, t, Li, np, np, 64, 0, 0, 1, 0, 0}); }
                    for (int r = TP; r < T; r++) { double *t = F + (int64_t)r * 64 * ld + 64 * p; h_gemm.push_back({t, t, Li, ld, ld, 64, 0, 0, 1, 0, 0}); }
                }
                gemm(sel_steps, b0);
            }
            size_t b0 = h_gemm.size();
            for (int s : sn) {    // Sigma_SB(j, i) = -sum_k Y(k, j)^T Sigma_BB(k, i)
                const int ld = P.ld(s), T = ld / 64, TP = P.NP[s] / 64;
                double *F = front(s);
                for (int j = 0; j < TP; j++)
                    for (int i = TP; i < T; i++)
                        h_gemm.push_back({F + (int64_t)j * 64 * ld + 64 * i, F + (int64_t)TP * 64 * ld + 64 * j, F + (int64_t)TP * 64 * ld + 64 * i, ld, ld, ld, 64 * ld, 64 * ld, T - TP, GI_TA | GI_NEG, 0});
            }
            gemm(sel_steps, b0);
            b0 = h_gemm.size();
            for (int s : sn) {    // Sigma_SS(i, j) = sum_{k >= max(i, j)} Z(k, i)^T Z(k, j)
                const int ld = P.ld(s), TP = P.NP[s] / 64, np = P.NP[s];
                double *F = front(s), *Z = ztile(s);
                for (int i = 0; i < TP; i++)
                    for (int j = 0; j < TP; j++) {
                        const int m = std::max(i, j);
                        h_gemm.push_back({F + (int64_t)i * 64 * ld + 64 * j, Z + (int64_t)m * 64 * np + 64 * i, Z + (int64_t)m * 64 * np + 64 * j, ld, np, np, 64 * np, 64 * np, TP - m, GI_TA, 0});
                    }
            }
            gemm(sel_steps, b0);
            b0 = h_gemm.size();
            for (int s : sn) {    // Sigma_SS(i, j) -= sum_k Sigma_SB(i, k) Y(k, j)
                const int ld = P.ld(s), T = ld / 64, TP = P.NP[s] / 64;
                if (T == TP) continue;
                double *F = front(s);
                for (int i = 0; i < TP; i++)
                    for (int j = 0; j < TP; j++)
                        h_gemm.push_back({F + (int64_t)i * 64 * ld + 64 * j, F + (int64_t)i * 64 * ld + 64 * TP, F + (int64_t)TP * 64 * ld + 64 * j, ld, ld, ld, 64, 64 * ld, T - TP, GI_ACC | GI_NEG, 0});
            }
            gemm(sel_steps, b0);
        }
        for (size_t k = sel_begin; k < h_gemm.size(); k++) selinv_flops += 2.0 * 64 * 64 * 64 * h_gemm[k].nk;
    }

    int upload_items(char *err, size_t errlen) {
        int rc;
        if ((rc = up(gemm_items, h_gemm.data(), h_gemm.size() * sizeof(GemmItem))) || (rc = up(diag_items, h_diag.data(), h_diag.size() * sizeof(DiagItem))) ||
            (rc = up(pairs, h_pairs.data(), h_pairs.size() * sizeof(EaPair)))) {
            snprintf(err, errlen, "uploading the sparse solver's item lists failed (%d)", rc);
            return rc;
        }
        std::vector<int32_t> kl;
        for (int s = plan.n_marg_sn; s < plan.nsn; s++) kl.push_back(s);
        n_kept_sn = (int)kl.size();
        if ((rc = up(kept_list, kl.data(), kl.size() * 4))) return rc;
        std::vector<GemmItem>().swap(h_gemm);
        std::vector<DiagItem>().swap(h_diag);
        std::vector<EaPair>().swap(h_pairs);
        return 0;
    }

    void run_steps(const std::vector<SpStep> &steps, hipStream_t s, int *bad) {
        for (const SpStep &st : steps) {
            switch (st.kind) {
            case SpStep::GEMM:
                hipLaunchKernelGGL(sp_gemm_items_kernel, dim3(st.count), dim3(256), 0, s, (const GemmItem *)gemm_items.p + st.begin);
                break;
            case SpStep::DIAG:
                hipLaunchKernelGGL(sp_diag_items_kernel, dim3(st.count), dim3(64), 0, s, (const DiagItem *)diag_items.p + st.begin, bad);
                break;
            case SpStep::EXTADD:
                by_dim(D, [&](auto d) { hipLaunchKernelGGL((sp_extend_add_kernel<decltype(d)::value>), dim3(st.count, st.ymax), dim3(256), 0, s, (const EaPair *)pairs.p + st.begin); });
                break;
            case SpStep::GATHER:
                by_dim(D, [&](auto d) { hipLaunchKernelGGL((sp_gather_sigma_kernel<decltype(d)::value>), dim3(st.count, st.ymax), dim3(256), 0, s, (const EaPair *)pairs.p + st.begin); });
                break;
            }
        }
    }

    // fronts <- H of the staged graph (gb.pos = D * elimination position), optionally b
    int assemble(hipStream_t s, const GraphBufs &gb, double *b, int *bad) {
        if (hipMemsetAsync(pool.p, 0, (size_t)std::max<int64_t>(plan.pool, 1) * 8, s) != hipSuccess) return SPG_EHIP;
        FrontSink sink{dev, bad ? bad : (int *)own_bad.p};
        by_dim(D, [&](auto d) { launch_assemble_into<decltype(d)::value>(gb, sink, s, b); });
        return 0;
    }
    // fronts <- the partial factorisations of the staged graph's H (no shift): the step the global KLD and the
    // covariance blocks share
    int factorise(hipStream_t s, const GraphBufs &gb, int *bad) {
        if (int rc = assemble(s, gb, nullptr, bad)) return rc;
        shift(s, 0.0, nullptr, 0);
        factor(s, bad);
        return 0;
    }
    // pivot diagonals += lambda, pads = 1; scal[slot] <- max |diag| before the shift (when scal != nullptr)
    void shift(hipStream_t s, double lambda, double *scal, int slot) {
        hipLaunchKernelGGL(sp_diag_shift_kernel, dim3(plan.nsn), dim3(64), 0, s, dev, lambda, scal ? (double *)partial.p : (double *)nullptr);
        if (scal) hipLaunchKernelGGL(sp_max_kernel, dim3(1), dim3(256), 0, s, (const double *)partial.p, plan.nsn, scal, slot);
    }
    // The launch sequence of a factorisation is fixed by the plan (a few hundred small launches): captured once into a
    // hipGraph and replayed for every LM trial. SPG_SPARSE_GRAPH=0 (or a failed capture) falls back to plain launches.
    hipGraphExec_t fact_graph = nullptr;
    int *fact_graph_bad = nullptr;
    bool graph_off = false;
    void factor(hipStream_t s, int *bad) {
        static const bool env_off = [] { const char *e = getenv("SPG_SPARSE_GRAPH"); return e && e[0] == '0'; }();
        if (env_off || graph_off || fact_steps.size() < 32) { run_steps(fact_steps, s, bad); return; }
        if (fact_graph && fact_graph_bad != bad) { (void)hipGraphExecDestroy(fact_graph); fact_graph = nullptr; }
        if (!fact_graph) {
            hipGraph_t gr = nullptr;
            if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); graph_off = true; run_steps(fact_steps, s, bad); return; }
            run_steps(fact_steps, s, bad);
            if (hipStreamEndCapture(s, &gr) != hipSuccess || !gr || hipGraphInstantiate(&fact_graph, gr, nullptr, nullptr, 0) != hipSuccess) {
                (void)hipGetLastError();
                if (gr) (void)hipGraphDestroy(gr);
                fact_graph = nullptr; graph_off = true;
                run_steps(fact_steps, s, bad);
                return;
            }
            (void)hipGraphDestroy(gr);
            fact_graph_bad = bad;
        }
        if (hipGraphLaunch(fact_graph, s) != hipSuccess) { (void)hipGetLastError(); graph_off = true; run_steps(fact_steps, s, bad); }
    }
    ~SparseSolver() { if (fact_graph) (void)hipGraphExecDestroy(fact_graph); }
    // a front's solve step is one workgroup streaming its panel: tall fronts (the top levels) get 16 wavefronts so that
    // enough loads are in flight, the many small ones keep 4
    int level_threads(int l) const {
        int tall = 0;
        for (int i = plan.level_ptr[l]; i < plan.level_ptr[l + 1]; i++) tall = std::max(tall, plan.ld(plan.level_sn[i]));
        return tall >= 768 ? 1024 : 256;
    }
    // x (length D * n, elimination order) <- H^-1 x
    void solve(hipStream_t s, double *x) {
        const Plan &P = plan;
        for (int l = 0; l < P.nlevels; l++)
            hipLaunchKernelGGL(sp_forward_kernel, dim3(P.level_ptr[l + 1] - P.level_ptr[l]), dim3(level_threads(l)), 0, s, dev, P.level_ptr[l], x);
        for (int l = P.nlevels - 1; l >= 0; l--)
            hipLaunchKernelGGL(sp_backward_kernel, dim3(P.level_ptr[l + 1] - P.level_ptr[l]), dim3(level_threads(l)), 0, s, dev, P.level_ptr[l], x, 0, (double *)nullptr);
    }
    // out[slot] <- sum over supernodes [s0, nsn) of sum log L_ii
    void logdiag(hipStream_t s, int s0, double *out, int slot) {
        hipLaunchKernelGGL(sp_logdiag_kernel, dim3(plan.nsn), dim3(64), 0, s, dev, (double *)partial.p);
        hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, s, (const double *)partial.p + s0, plan.nsn - s0, out, slot);
    }
    // out[slot] <- || L^T x ||^2
    void ltx_norm2(hipStream_t s, double *x, double *out, int slot) {
        const Plan &P = plan;
        for (int l = 0; l < P.nlevels; l++)
            hipLaunchKernelGGL(sp_backward_kernel, dim3(P.level_ptr[l + 1] - P.level_ptr[l]), dim3(level_threads(l)), 0, s, dev, P.level_ptr[l], x, 1, (double *)partial.p);
        hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, s, (const double *)partial.p, P.nsn, out, slot);
    }
    // stats += what this solver (initialised with_selinv) costs: supernodes, bytes of fronts and Z blocks, flops
    void count_into(spg_cov_stats &st) const {
        st.supernodes += plan.nsn; st.front_bytes += (double)(plan.pool + zpool_len) * 8;
        st.factor_flops += plan.flops; st.selinv_flops += selinv_flops;
    }
    int selected_inverse(hipStream_t s, int *bad) {
        if (hipMemsetAsync(zpool.p, 0, (size_t)std::max<int64_t>(zpool_len, 1) * 8, s) != hipSuccess) return SPG_EHIP;
        if (n_kept_sn > 0)
            hipLaunchKernelGGL(sp_z_identity_kernel, dim3(n_kept_sn), dim3(256), 0, s, (double *)zpool.p, d_zoff, dev.NP, (const int32_t *)kept_list.p, n_kept_sn);
        run_steps(sel_steps, s, bad);
        return 0;
    }
};

// block adjacency of the free vertices of a staged graph; blocks are numbered by ascending in.pos
void block_graph_of(const spg::DenseGraphIn &in, const std::vector<int32_t> &block_of, int nblocks, spg::sparse::BlockGraph &g) {
    std::vector<std::pair<int32_t, int32_t>> pr;
    for (int e = 0; e < in.ne; e++) {
        const spg_edge_ref &er = in.er[e];
        for (int i = 0; i < er.nv; i++) {
            const int bi = block_of[in.ev[er.vbegin + i]];
            if (bi < 0) continue;
            for (int j = i + 1; j < er.nv; j++) {
                const int bj = block_of[in.ev[er.vbegin + j]];
                if (bj < 0 || bj == bi) continue;
                pr.push_back({bi, bj});
                pr.push_back({bj, bi});
            }
        }
    }
    std::sort(pr.begin(), pr.end());
    pr.erase(std::unique(pr.begin(), pr.end()), pr.end());
    g.n = nblocks;
    g.ptr.assign((size_t)nblocks + 1, 0);
    g.adj.resize(pr.size());
    for (auto &p : pr) g.ptr[p.first + 1]++;
    for (int i = 0; i < nblocks; i++) g.ptr[i + 1] += g.ptr[i];
    for (size_t i = 0; i < pr.size(); i++) g.adj[i] = pr[i].second;
}

int sparse_leaf(int D) {
    const char *e = getenv("SPG_SPARSE_LEAF");
    int v = e ? atoi(e) : 0;
    return v > 0 ? v : (D == 6 ? 32 : 64);
}

// Plan of a staged graph: blocks = its free vertices numbered by ascending in.pos, is_marg_vertex (per vertex, or null)
// = the blocks to eliminate first; pos[v] = D * elimination position of vertex v, -1 for the others.
void plan_of(const spg::DenseGraphIn &in, const uint8_t *is_marg_vertex, spg::sparse::Plan &plan, std::vector<int32_t> &pos) {
    std::vector<int32_t> blk((size_t)in.nv, -1);
    int nb = 0;
    {
        std::vector<std::pair<int32_t, int32_t>> order;
        for (int v = 0; v < in.nv; v++) if (in.pos[v] >= 0) order.push_back({in.pos[v], v});
        std::sort(order.begin(), order.end());
        for (auto &p : order) blk[p.second] = nb++;
    }
    std::vector<uint8_t> im;
    if (is_marg_vertex) {
        im.assign((size_t)nb, 0);
        for (int v = 0; v < in.nv; v++) if (blk[v] >= 0 && is_marg_vertex[v]) im[blk[v]] = 1;
    }
    spg::sparse::BlockGraph bg;
    block_graph_of(in, blk, nb, bg);
    spg::sparse::build_plan(bg, in.D, is_marg_vertex ? im.data() : nullptr, sparse_leaf(in.D), plan);
    pos.assign((size_t)in.nv, -1);
    for (int v = 0; v < in.nv; v++) if (blk[v] >= 0) pos[v] = in.D * plan.iperm[blk[v]];
}

// ---- columns of Sigma through the fronts (host half of sp_panel_rows_kernel & co.)
// Sigma[:, b] = L^-T L^-1 E_b. The forward sweep of E_b is non-zero only on the fronts of the path from b's supernode to
// the root; the backward sweep restricted to the rows of a vertex a needs only the path from the root down to a's
// supernode (boundary values are the ancestors' solved unknowns, gathered from the parent's panel). A batch of columns
// therefore runs over the union of those paths only, level by level like the single-RHS solves, and must run on the
// intact factor: before selected_inverse, which overwrites L_SS and L_BS (the diagonal-tile inverses survive).
bool cov_force_solve() {
    static const bool v = [] { const char *e = getenv("SPG_COV_FORCE_SOLVE"); return e && e[0] == '1'; }();
    return v;
}

// the device flags of the covariance drivers: [0] a pivot failed, [1] a request fell outside the fronts
int cov_bad_flags(const int *h_bad, char *err, size_t errlen) {
    if (h_bad[0]) { snprintf(err, errlen, "covariance blocks: the information matrix is not positive definite"); return SPG_ENOTPD; }
    if (h_bad[1]) { snprintf(err, errlen, "covariance blocks: a requested pair lies outside the fronts of the factorisation"); return SPG_ESTATE; }
    return 0;
}

// block (qa, qb) of positions lies inside the fronts, where FrontSink::locate finds Sigma after the selected inverse
bool in_fronts(const Plan &P, int qa, int qb) {
    const int qu = std::min(qa, qb), qv = std::max(qa, qb), s = P.sn_of[qu];
    if (qv < P.first[s + 1]) return true;
    return std::binary_search(P.rows.begin() + P.rowptr[s], P.rows.begin() + P.rowptr[s + 1], qv);
}

// Greedy column cover: request i = block pair (x[i], y[i]) needs the column of x[i] or of y[i]; the block with the most
// uncovered requests is solved first (ties: the earlier position), a diagonal request (x == y) needs its own column.
void choose_columns(int nblocks, const std::vector<int32_t> &x, const std::vector<int32_t> &y, std::vector<int32_t> &col) {
    const size_t m = x.size();
    std::vector<int32_t> deg((size_t)nblocks, 0), ptr((size_t)nblocks + 1, 0), inc;
    for (size_t i = 0; i < m; i++) { ptr[x[i] + 1]++; if (y[i] != x[i]) ptr[y[i] + 1]++; }
    for (int v = 0; v < nblocks; v++) { deg[v] = ptr[v + 1]; ptr[v + 1] += ptr[v]; }
    inc.resize((size_t)ptr[nblocks]);
    {
        std::vector<int32_t> f(ptr.begin(), ptr.end() - 1);
        for (size_t i = 0; i < m; i++) { inc[f[x[i]]++] = (int32_t)i; if (y[i] != x[i]) inc[f[y[i]]++] = (int32_t)i; }
    }
    col.assign(m, -1);
    auto take = [&](int v) {
        for (int32_t k = ptr[v]; k < ptr[v + 1]; k++) {
            const int32_t i = inc[k];
            if (col[i] >= 0) continue;
            col[i] = v;
            const int o = x[i] == v ? y[i] : x[i];
            if (o != v) deg[o]--;
        }
        deg[v] = 0;
    };
    for (size_t i = 0; i < m; i++) if (x[i] == y[i] && col[i] < 0) take(x[i]);
    std::priority_queue<std::pair<int32_t, int32_t>> pq;
    for (int v = 0; v < nblocks; v++) if (deg[v] > 0) pq.push({deg[v], -v});
    while (!pq.empty()) {
        const auto [d, nv] = pq.top();
        pq.pop();
        const int v = -nv;
        if (deg[v] == 0) continue;
        if (deg[v] != d) { pq.push({deg[v], -v}); continue; }
        take(v);
    }
}

// HIPCHK in the wording of the column solves' messages
#define COLCHK(what, x)                                                                                                  \
    do {                                                                                                                 \
        hipError_t e_ = (x);                                                                                             \
        if (e_ != hipSuccess) {                                                                                          \
            snprintf(err, errlen, "covariance column solves: %s failed: %s", what, hipGetErrorString(e_));             \
            return SPG_EHIP;                                                                                             \
        }                                                                                                                \
    } while (0)

struct ColumnSolves {
    enum Kind { GEMM, EXTADD, GATHER, SEED, CROSS };
    struct Step { Kind kind; int64_t begin; int32_t count, gy, gz; };
    SparseSolver &sp;
    const Plan &P;
    int D;
    // requests: Sigma[row block, column block] -> cross[i]
    std::vector<int32_t> cols;                  // column blocks, ascending position
    std::vector<int32_t> rq_ptr, rq_row, rq_idx;  // per column: its requests' row blocks and cross indices
    int per_batch = 1, nbatch = 0;
    double flops = 0, seconds = 0;
    std::vector<int32_t> fw, bw, stamp_list;
    std::vector<int32_t> bw_always;   // supernodes every batch sweeps backward over (the lazy greedy rounds: the paths of all of S)
    int32_t stamp = 0;
    std::vector<int64_t> off;
    ColumnSolves(SparseSolver &s_, const std::vector<int32_t> &row, const std::vector<int32_t> &col) : sp(s_), P(s_.plan), D(s_.D) {
        const size_t m = row.size();
        std::vector<int32_t> order(m);
        for (size_t i = 0; i < m; i++) order[i] = (int32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return col[a] < col[b]; });
        rq_ptr.push_back(0);
        for (size_t k = 0; k < m; k++) {
            const int32_t i = order[k];
            if (cols.empty() || cols.back() != col[i]) { if (!cols.empty()) rq_ptr.push_back((int32_t)rq_row.size()); cols.push_back(col[i]); }
            rq_row.push_back(row[i]);
            rq_idx.push_back(i);
        }
        if (!cols.empty()) rq_ptr.push_back((int32_t)rq_row.size());
        fw.assign((size_t)P.nsn, 0);
        bw.assign((size_t)P.nsn, 0);
        off.assign((size_t)P.nsn, -1);
    }
    int width(int b) const {   // panel width of batch b: D columns per column vertex, padded to 64
        const int nc = std::min<int>(per_batch, (int)cols.size() - b * per_batch);
        return (D * nc + 63) / 64 * 64;
    }
    // marks fw / bw with the current stamp; returns the panel scalars of the batch
    int64_t touch(int b) {
        stamp++;
        const int c0 = b * per_batch, c1 = std::min<int>(c0 + per_batch, (int)cols.size());
        auto up = [&](std::vector<int32_t> &mk, int q) {
            for (int s = P.sn_of[q]; s >= 0 && mk[s] != stamp; s = P.parent[s]) mk[s] = stamp;
        };
        for (int c = c0; c < c1; c++) {
            up(fw, cols[c]);
            for (int32_t k = rq_ptr[c]; k < rq_ptr[c + 1]; k++) up(bw, rq_row[k]);
        }
        for (int32_t s : bw_always) bw[s] = stamp;
        const int R = width(b);
        int64_t len = 0;
        for (int s : P.level_sn)
            if (fw[s] == stamp || bw[s] == stamp) { off[s] = len; len += (int64_t)P.ld(s) * R; }
        return len;
    }
    // panel width R_max (a multiple of 64 up to 512) and the largest batch workspace that fits in free HBM
    int plan_batches(int64_t &ws_len, char *err, size_t errlen) {
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        const double avail = (double)free_b - (double)(1ull << 30);
        for (int Rm = 512; Rm >= 64; Rm /= 2) {
            per_batch = std::max(1, Rm / D);
            nbatch = ((int)cols.size() + per_batch - 1) / per_batch;
            ws_len = 0;
            for (int b = 0; b < nbatch; b++) ws_len = std::max(ws_len, touch(b));
            if ((double)ws_len * 8 + 64.0 * 1e6 <= avail) return 0;
        }
        snprintf(err, errlen, "covariance column solves: the right-hand-side panels of one batch need %.2f GB, %.2f GB of HBM are free",
                 ws_len * 8e-9, free_b * 1e-9);
        return SPG_ECAPACITY;
    }
    // host item lists of batch b over the panel workspace ws
    std::vector<GemmItem> gi;
    std::vector<PanelPair> pp;
    std::vector<int64_t> seeds, csrc;
    std::vector<int32_t> cdst;
    std::vector<Step> steps;
    void build(int b, double *ws) {
        gi.clear(); pp.clear(); seeds.clear(); csrc.clear(); cdst.clear(); steps.clear();
        touch(b);
        const int R = width(b), CT = R / 64, c0 = b * per_batch, c1 = std::min<int>(c0 + per_batch, (int)cols.size());
        const double *linv = (const double *)sp.linv.p;
        auto W = [&](int s) { return ws + off[s]; };
        auto F = [&](int s) { return (const double *)sp.front(s); };
        auto gemm = [&](size_t b0) { if (gi.size() > b0) steps.push_back({GEMM, (int64_t)b0, (int32_t)(gi.size() - b0), 0, 0}); };
        auto rows_step = [&](Kind k, size_t b0, int maxrows) {
            if (pp.size() > b0) steps.push_back({k, (int64_t)b0, (int32_t)(pp.size() - b0), CT, (maxrows + 63) / 64});
        };
        for (int c = c0; c < c1; c++) {
            const int q = cols[c], s = P.sn_of[q], j = c - c0;
            for (int d = 0; d < D; d++) seeds.push_back(off[s] + (int64_t)(D * (q - P.first[s]) + d) * R + D * j + d);
        }
        steps.push_back({SEED, 0, (int32_t)seeds.size(), 0, 0});
        std::vector<int> lv;
        // forward: L y = E over the columns' root paths
        for (int l = 0; l < P.nlevels; l++) {
            lv.clear();
            for (int i = P.level_ptr[l]; i < P.level_ptr[l + 1]; i++) if (fw[P.level_sn[i]] == stamp) lv.push_back(P.level_sn[i]);
            if (lv.empty()) continue;
            for (int k = 0;; k++) {   // the children's update rows, child rank by child rank
                const size_t b0 = pp.size();
                int maxrows = 0;
                bool more = false;
                for (int s : lv) {
                    int rank = 0;
                    for (int ci = P.childptr[s]; ci < P.childptr[s + 1]; ci++) {
                        const int ch = P.child[ci];
                        if (fw[ch] != stamp) continue;
                        if (rank++ != k) { if (rank > k + 1) { more = true; break; } continue; }
                        pp.push_back({W(ch) + (int64_t)P.NP[ch] * R, W(s), sp.dev.rel + P.rowptr[ch], D * P.nrows(ch), R});
                        maxrows = std::max(maxrows, D * P.nrows(ch));
                    }
                }
                rows_step(EXTADD, b0, maxrows);
                if (!more) break;
            }
            int maxtp = 0;
            for (int s : lv) maxtp = std::max(maxtp, P.NP[s] / 64);
            for (int p = 0; p < maxtp; p++) {
                size_t b0 = gi.size();
                if (p > 0)   // y_p -= sum_{q < p} L(p, q) y_q
                    for (int s : lv) {
                        if (P.NP[s] / 64 <= p) continue;
                        const int ld = P.ld(s);
                        for (int c = 0; c < CT; c++)
                            gi.push_back({W(s) + (int64_t)p * 64 * R + 64 * c, F(s) + (int64_t)p * 64 * ld, W(s) + 64 * c, R, ld, R, 64, 64 * R, p, GI_ACC | GI_NEG, 0});
                    }
                gemm(b0);
                b0 = gi.size();
                for (int s : lv) {   // y_p = L_pp^-1 y_p (in place: one K tile, read before written)
                    if (P.NP[s] / 64 <= p) continue;
                    for (int c = 0; c < CT; c++) {
                        double *t = W(s) + (int64_t)p * 64 * R + 64 * c;
                        gi.push_back({t, linv + P.loff[s] + (int64_t)p * 4096, t, R, 64, R, 0, 0, 1, 0, 0});
                    }
                }
                gemm(b0);
            }
            const size_t b0 = gi.size();
            for (int s : lv) {   // update rows for the parent: u -= L_BS y_S
                const int ld = P.ld(s), T = ld / 64, TP = P.NP[s] / 64;
                for (int r = TP; r < T; r++)
                    for (int c = 0; c < CT; c++)
                        gi.push_back({W(s) + (int64_t)r * 64 * R + 64 * c, F(s) + (int64_t)r * 64 * ld, W(s) + 64 * c, R, ld, R, 64, 64 * R, TP, GI_ACC | GI_NEG, 0});
            }
            gemm(b0);
        }
        // backward: L^T x = y over the requested rows' root paths, top-down
        for (int l = P.nlevels - 1; l >= 0; l--) {
            lv.clear();
            for (int i = P.level_ptr[l]; i < P.level_ptr[l + 1]; i++) if (bw[P.level_sn[i]] == stamp) lv.push_back(P.level_sn[i]);
            if (lv.empty()) continue;
            {
                const size_t b0 = pp.size();
                int maxrows = 0;
                for (int s : lv) {
                    if (P.parent[s] < 0 || P.nrows(s) == 0) continue;
                    pp.push_back({W(s) + (int64_t)P.NP[s] * R, W(P.parent[s]), sp.dev.rel + P.rowptr[s], D * P.nrows(s), R});
                    maxrows = std::max(maxrows, D * P.nrows(s));
                }
                rows_step(GATHER, b0, maxrows);
            }
            int maxtp = 0;
            for (int s : lv) maxtp = std::max(maxtp, P.NP[s] / 64);
            for (int st = 0; st < maxtp; st++) {
                size_t b0 = gi.size();
                for (int s : lv) {   // x_p = y_p - sum_{r > p} L(r, p)^T x_r
                    const int ld = P.ld(s), T = ld / 64, TP = P.NP[s] / 64;
                    if (TP <= st) continue;
                    const int p = TP - 1 - st;
                    if (T - p - 1 == 0) continue;
                    for (int c = 0; c < CT; c++)
                        gi.push_back({W(s) + (int64_t)p * 64 * R + 64 * c, F(s) + (int64_t)(p + 1) * 64 * ld + 64 * p, W(s) + (int64_t)(p + 1) * 64 * R + 64 * c,
                                      R, ld, R, 64 * ld, 64 * R, T - p - 1, GI_TA | GI_ACC | GI_NEG, 0});
                }
                gemm(b0);
                b0 = gi.size();
                for (int s : lv) {   // x_p = L_pp^-T x_p
                    const int TP = P.NP[s] / 64;
                    if (TP <= st) continue;
                    const int p = TP - 1 - st;
                    for (int c = 0; c < CT; c++) {
                        double *t = W(s) + (int64_t)p * 64 * R + 64 * c;
                        gi.push_back({t, linv + P.loff[s] + (int64_t)p * 4096, t, R, 64, R, 0, 0, 1, GI_TA, 0});
                    }
                }
                gemm(b0);
            }
        }
        for (int c = c0; c < c1; c++)
            for (int32_t k = rq_ptr[c]; k < rq_ptr[c + 1]; k++) {
                const int q = rq_row[k], s = P.sn_of[q];
                csrc.push_back(off[s] + (int64_t)D * (q - P.first[s]) * R + D * (c - c0));
                cdst.push_back(rq_idx[k]);
            }
        steps.push_back({CROSS, 0, (int32_t)csrc.size(), 0, 0});
        for (const GemmItem &it : gi) flops += 2.0 * 64 * 64 * 64 * it.nk;
    }
    // every batch: panels zeroed, seeded, forward, backward, requested rows -> cross (n requests x D^2)
    int run(hipStream_t s, double *cross, char *err, size_t errlen) {
        int64_t ws_len = 0;
        if (cols.empty()) return 0;
        if (int rc = plan_batches(ws_len, err, errlen)) return rc;
        DevBuf ws, blob;
        size_t blob_cap = 0;
        std::vector<char> hb;
        if (hipMalloc(&ws.p, (size_t)std::max<int64_t>(ws_len, 1) * 8) != hipSuccess) {
            snprintf(err, errlen, "covariance column solves: hipMalloc of %.2f GB of panels failed", ws_len * 8e-9);
            return SPG_ECAPACITY;
        }
        EventTimer timer;   // one batch at a time
        float ms = 0;
        for (int b = 0; b < nbatch; b++)
            if (int rc = enqueue(s, b, ws, blob, blob_cap, hb, timer, b > 0, cross, err, errlen)) return rc;
        COLCHK("a batch", hipStreamSynchronize(s));
        COLCHK("hipEventElapsedTime", timer.ms(ms));
        seconds += 1e-3 * ms;
        return 0;
    }
    // Batch b into the stream, inside the timer's event pair: item lists built and uploaded (the blob grows as needed), the
    // panels of ws zeroed and seeded, forward, backward, the requested rows -> cross. wait_prev: the stream still runs a
    // batch that reads the blob and the panels; it is waited for and its time is added to `seconds` first.
    int enqueue(hipStream_t s, int b, DevBuf &ws, DevBuf &blob, size_t &blob_cap, std::vector<char> &hb, EventTimer &timer, bool wait_prev, double *cross,
                char *err, size_t errlen) {
        build(b, (double *)ws.p);
        // one upload per batch: gemm items | panel pairs | seeds | cross sources | cross destinations
        const size_t o_pp = gi.size() * sizeof(GemmItem), o_sd = o_pp + pp.size() * sizeof(PanelPair), o_cs = o_sd + seeds.size() * 8,
                     o_cd = o_cs + csrc.size() * 8, nbytes = o_cd + cdst.size() * 4;
        hb.resize(nbytes);
        memcpy(hb.data(), gi.data(), o_pp);
        memcpy(hb.data() + o_pp, pp.data(), o_sd - o_pp);
        memcpy(hb.data() + o_sd, seeds.data(), o_cs - o_sd);
        memcpy(hb.data() + o_cs, csrc.data(), o_cd - o_cs);
        memcpy(hb.data() + o_cd, cdst.data(), nbytes - o_cd);
        if (wait_prev) {
            float ms = 0;
            COLCHK("a batch", hipStreamSynchronize(s));
            COLCHK("hipEventElapsedTime", timer.ms(ms));
            seconds += 1e-3 * ms;
        }
        if (nbytes > blob_cap) {
            if (blob.p) { (void)hipFree(blob.p); blob.p = nullptr; }
            blob_cap = nbytes + nbytes / 4;
            COLCHK("hipMalloc of the item lists", hipMalloc(&blob.p, blob_cap));
        }
        COLCHK("uploading the item lists", hipMemcpy(blob.p, hb.data(), nbytes, hipMemcpyHostToDevice));
        const char *B = (const char *)blob.p;
        const int R = width(b);
        int64_t len = 0;
        for (int sn : P.level_sn) if (fw[sn] == stamp || bw[sn] == stamp) len += (int64_t)P.ld(sn) * R;
        COLCHK(timer.made != hipSuccess ? "hipEventCreate" : "hipEventRecord", timer.start(s));
        COLCHK("hipMemsetAsync", hipMemsetAsync(ws.p, 0, (size_t)std::max<int64_t>(len, 1) * 8, s));
        for (const Step &st : steps) {
            const PanelPair *pairs = (const PanelPair *)(B + o_pp) + st.begin;
            switch (st.kind) {
            case GEMM:
                hipLaunchKernelGGL(sp_gemm_items_kernel, dim3(st.count), dim3(256), 0, s, (const GemmItem *)B + st.begin);
                break;
            case EXTADD:
                by_dim(D, [&](auto d) { hipLaunchKernelGGL((sp_panel_rows_kernel<decltype(d)::value, false>), dim3(st.count, st.gy, st.gz), dim3(256), 0, s, pairs); });
                break;
            case GATHER:
                by_dim(D, [&](auto d) { hipLaunchKernelGGL((sp_panel_rows_kernel<decltype(d)::value, true>), dim3(st.count, st.gy, st.gz), dim3(256), 0, s, pairs); });
                break;
            case SEED:
                hipLaunchKernelGGL(sp_panel_seed_kernel, dim3((st.count + 255) / 256), dim3(256), 0, s, (double *)ws.p, (const int64_t *)(B + o_sd), st.count);
                break;
            case CROSS:
                if (st.count > 0)
                    hipLaunchKernelGGL(sp_cross_rows_kernel, dim3((st.count * D * D + 255) / 256), dim3(256), 0, s, (const double *)ws.p, (const int64_t *)(B + o_cs),
                                       (const int32_t *)(B + o_cd), st.count, D, R, cross);
                break;
            }
        }
        COLCHK("a launch", hipGetLastError());
        COLCHK("hipEventRecord", timer.stop(s));
        return 0;
    }
};

// The per-round column solves of the lazy greedy calls (DESIGN 5g-L) and the column cache they fill. One 64-wide panel
// per round: forward over the root paths of the new column vertices, backward over the paths of all of S — the same set
// every round, marked once (bw_always), so the panel layout, the workspace and the rows the strips are read from are fixed
// for the call. SPG_GREEDY_CACHE_STRIPS=<n> (diagnostic) caps the cache at n >= 2 strips.
struct LazySweeps {
    static const std::vector<int32_t> &none() { static const std::vector<int32_t> v; return v; }
    ColumnSolves cs;
    const int D, m;
    std::vector<int32_t> q;          // per endpoint slot: block position
    DevBuf ws, blob, dsrow, dstrip, cache;
    size_t blob_cap = 0;
    std::vector<char> hb;
    EventTimer timer;
    bool pending = false;            // a panel is in the stream whose time has not been read
    long long strip_len = 0;
    int nstrips = 0, batches = 0;
    LazySweeps(SparseSolver &sp, std::vector<int32_t> q_) : cs(sp, none(), none()), D(sp.D), m((int)q_.size()), q(std::move(q_)) {}
    // reserved: bytes the caller has yet to allocate. The cache takes what is left of free HBM (1 GB kept free), at most m
    // strips and at most max_strips, what the rounds of the call can fill.
    int init(double reserved, long long max_strips, char *err, size_t errlen) {
        const Plan &P = cs.P;
        std::vector<uint8_t> mk((size_t)P.nsn, 0);
        for (int32_t v : q)
            for (int sn = P.sn_of[v]; sn >= 0 && !mk[sn]; sn = P.parent[sn]) { mk[sn] = 1; cs.bw_always.push_back(sn); }
        cs.per_batch = spg::kGreedyPanel / D;
        cs.nbatch = 1;
        cs.cols.assign(1, q[0]);
        cs.rq_ptr.assign(2, 0);
        const int64_t ws_len = cs.touch(0);
        strip_len = (long long)m * D * D;
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        const double avail = (double)free_b - (double)(1ull << 30) - reserved - (double)ws_len * 8 - 64.0e6;
        long long fit = avail <= 0 ? 0 : (long long)(avail / ((double)strip_len * 8));
        if (const char *e = getenv("SPG_GREEDY_CACHE_STRIPS")) { const int v = atoi(e); if (v > 0) fit = std::min<long long>(fit, std::max(2, v)); }
        if (fit < 2) {
            snprintf(err, errlen, "lazy greedy rounds need a %.2f GB panel workspace and two %.2f GB column strips, %.2f GB of HBM are free",
                     ws_len * 8e-9, strip_len * 8e-9, free_b * 1e-9);
            return SPG_ECAPACITY;
        }
        nstrips = (int)std::min<long long>(fit, std::max<long long>(2, std::min<long long>(m, max_strips)));
        COLCHK("hipMalloc of the panel workspace", hipMalloc(&ws.p, (size_t)std::max<int64_t>(ws_len, 1) * 8));
        COLCHK("hipMalloc of the column cache", hipMalloc(&cache.p, (size_t)nstrips * strip_len * 8));
        COLCHK("hipMalloc", hipMalloc(&dstrip.p, spg::kGreedyPanel * sizeof(int32_t)));
        std::vector<int64_t> srow((size_t)m);
        for (int j = 0; j < m; j++) { const int sn = P.sn_of[q[j]]; srow[j] = cs.off[sn] + (int64_t)D * (q[j] - P.first[sn]) * spg::kGreedyPanel; }
        COLCHK("hipMalloc", hipMalloc(&dsrow.p, (size_t)m * 8));
        COLCHK("uploading the strip rows", hipMemcpy(dsrow.p, srow.data(), (size_t)m * 8, hipMemcpyHostToDevice));
        return 0;
    }
    double cache_bytes() const { return (double)nstrips * strip_len * 8; }
    // after a synchronisation of the stream: the time of the panel in flight
    int collect(char *err, size_t errlen) {
        if (!pending) return 0;
        float ms = 0;
        COLCHK("hipEventElapsedTime", timer.ms(ms));
        cs.seconds += 1e-3 * ms;
        pending = false;
        return 0;
    }
    // The columns of gr.solve_vertex into the strips gr.solve_strip. The stream is idle: the caller has read the round's
    // control words.
    int solve(hipStream_t s, const spg::GreedyRound &gr, char *err, size_t errlen) {
        const int nc = (int)gr.solve_vertex.size();
        if (nc == 0) return 0;
        cs.cols.resize((size_t)nc);
        for (int c = 0; c < nc; c++) cs.cols[c] = q[gr.solve_vertex[c]];
        cs.rq_ptr.assign((size_t)nc + 1, 0);
        COLCHK("uploading the strip slots", hipMemcpy(dstrip.p, gr.solve_strip.data(), (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice));
        if (int rc = cs.enqueue(s, 0, ws, blob, blob_cap, hb, timer, false, nullptr, err, errlen)) return rc;
        pending = true;
        batches++;
        const long long total = (long long)m * D * D * nc;
        hipLaunchKernelGGL(sp_strip_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const double *)ws.p, (const int64_t *)dsrow.p, m, D,
                           spg::kGreedyPanel, (const int32_t *)dstrip.p, nc, strip_len, (double *)cache.p);
        COLCHK("a launch", hipGetLastError());
        return 0;
    }
};

// Sparse linear algebra for LM: the fronts are re-assembled for every trial (the estimates of a trial are those
// of its iteration), shifted by lambda, factorised, and the right-hand side is solved in place.
struct SparseLM : LMLinear {
    SparseSolver sp;
    int nvec = 0;
    bool fresh = false;   // the pool holds the unshifted H of the current estimates
    int build(hipStream_t s, const GraphBufs &gb, double *b, double *scal, char *err, size_t errlen) override {
        int rc = sp.assemble(s, gb, b, nullptr);
        if (rc) { snprintf(err, errlen, "sparse assembly failed"); return rc; }
        sp.shift(s, 0.0, scal, 1);
        fresh = true;
        return 0;
    }
    int solve(hipStream_t s, const GraphBufs &gb, double lambda, const double *b, double *sol, int *bad, char *err, size_t errlen) override {
        if (!fresh) {
            int rc = sp.assemble(s, gb, nullptr, bad);
            if (rc) { snprintf(err, errlen, "sparse assembly failed"); return rc; }
        }
        fresh = false;
        sp.shift(s, lambda, nullptr, 0);
        sp.factor(s, bad);
        if (hipMemcpyAsync(sol, b, (size_t)nvec * 8, hipMemcpyDeviceToDevice, s) != hipSuccess) return SPG_EHIP;
        sp.solve(s, sol);
        return 0;
    }
};

}  // namespace

namespace spg {

// Plan of a block graph given as CSR (host debugging / CPU tests of the symbolic phase: tests/test_sparse_plan.py).
int sparse_plan_debug(int n, const int32_t *ptr, const int32_t *adj, int D, const uint8_t *is_marg, int leaf, spg::sparse::Plan &out) {
    spg::sparse::BlockGraph g;
    g.n = n;
    g.ptr.assign(ptr, ptr + n + 1);
    g.adj.assign(adj, adj + ptr[n]);
    spg::sparse::build_plan(g, D, is_marg, leaf > 0 ? leaf : sparse_leaf(D), out);
    return 0;
}

// optimize() with the sparse solver. in.pos: >= 0 for every free vertex (any distinct values; their order numbers the
// blocks), -1 otherwise. On return the arena holds the optimised estimates.
int hip_sparse_optimize(void *stream, const DenseGraphIn &in_, int n, int iterations, spg_optimize_stats &out, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    const int D = in_.D, nb = n / D;
    // blocks by ascending pos
    std::vector<int32_t> block_of((size_t)in_.nv, -1), pos_new((size_t)in_.nv, -1);
    {
        std::vector<std::pair<int32_t, int32_t>> order;
        for (int v = 0; v < in_.nv; v++) if (in_.pos[v] >= 0) order.push_back({in_.pos[v], v});
        std::sort(order.begin(), order.end());
        if ((int)order.size() != nb) { snprintf(err, errlen, "hip_sparse_optimize: %d free vertices, n = %d", (int)order.size(), n); return SPG_EINVAL; }
        for (int i = 0; i < nb; i++) block_of[order[i].second] = i;
    }
    sparse::BlockGraph bg;
    block_graph_of(in_, block_of, nb, bg);
    sparse::Plan plan;
    sparse::build_plan(bg, D, nullptr, sparse_leaf(D), plan);
    for (int v = 0; v < in_.nv; v++) if (block_of[v] >= 0) pos_new[v] = D * plan.iperm[block_of[v]];
    DenseGraphIn in = in_;
    in.pos = pos_new.data();
    auto lin = std::make_unique<SparseLM>();
    out.supernodes += plan.nsn; out.front_bytes += (double)plan.pool * 8; out.factor_flops += plan.flops;
    int rc = lin->sp.init(std::move(plan), false, err, errlen);
    if (rc) return rc;
    lin->nvec = std::max(n, 1);
    GraphBufs gb;
    if ((rc = stage_graph(in, gb, s))) { snprintf(err, errlen, "staging the graph for the optimiser failed (%d)", rc); return rc; }
    return lm_run(s, in, gb, n, lin->nvec, iterations, *lin, out, err, errlen);
}

// Global KLD with the sparse solver. base.pos: >= 0 for the baseline's free vertices (ascending = the caller's order),
// is_marg_vertex[v] = 1 for the ones the sparsified graph lacks; other.pos >= 0 for other's free vertices;
// kept_*: the common vertices as indices into the two graphs (same order), with their pose offsets.
int hip_sparse_kld(void *stream, const DenseGraphIn &base_, const DenseGraphIn &other_, const uint8_t *is_marg_vertex,
                   const int32_t *kept_b, const int32_t *kept_o, int nk, const int64_t *kept_vpo_base, const int64_t *kept_vpo_other,
                   spg_kld_terms &terms, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    int rc = 0;
    const int D = base_.D;
    // ---- plans
    sparse::Plan pb, po;
    std::vector<int32_t> pos_b, pos_o, pos_ob((size_t)other_.nv, -1);
    plan_of(base_, is_marg_vertex, pb, pos_b);
    plan_of(other_, nullptr, po, pos_o);
    for (int i = 0; i < nk; i++) pos_ob[kept_o[i]] = pos_b[kept_b[i]];    // other's vertices at the baseline's positions
    terms.supernodes += pb.nsn; terms.front_bytes += (double)(pb.pool + po.pool) * 8; terms.factor_flops += pb.flops + po.flops;
    const int n_marg_sn = pb.n_marg_sn;
    auto sb = std::make_unique<SparseSolver>(), so = std::make_unique<SparseSolver>();
    if ((rc = sb->init(std::move(pb), true, err, errlen)) || (rc = so->init(std::move(po), false, err, errlen))) return rc;
    DenseGraphIn base = base_, other = other_, other_at_base = other_;
    base.pos = pos_b.data();
    other.pos = pos_o.data();
    other_at_base.pos = pos_ob.data();
    GraphBufs gbb, gbo, gbx;
    DevBuf bad, outb, diff, tpart, vb, vo, dpos;
    std::vector<int32_t> kpos((size_t)nk);
    for (int i = 0; i < nk; i++) kpos[i] = pos_o[kept_o[i]];
    HIPCHK(hipMalloc(&bad.p, 2 * sizeof(int)));
    HIPCHK(hipMalloc(&outb.p, 8 * 8));
    HIPCHK(hipMalloc(&diff.p, (size_t)std::max(nk, 1) * D * 8 * 2));
    HIPCHK(hipMalloc(&tpart.p, (size_t)std::max(other_.nv, 1) * 8));
    EventTimer timer;
    if ((rc = upload(vb, kept_vpo_base, (size_t)nk, s)) || (rc = upload(vo, kept_vpo_other, (size_t)nk, s)) || (rc = upload(dpos, kpos.data(), (size_t)nk, s)) ||
        (rc = stage_graph(base, gbb, s)) || (rc = stage_graph(other, gbo, s)) || (rc = stage_graph(other_at_base, gbx, s))) {
        snprintf(err, errlen, "staging the graphs for the sparse KLD failed (%d)", rc);
        return rc;
    }
    HIPCHK(timer.start(s));
    HIPCHK(hipMemsetAsync(bad.p, 0, 2 * sizeof(int), s));
    HIPCHK(hipMemsetAsync(tpart.p, 0, (size_t)std::max(other_.nv, 1) * 8, s));
    int *bad0 = (int *)bad.p, *bad1 = (int *)bad.p + 1;
    double *out = (double *)outb.p, *dk = (double *)diff.p, *dperm = (double *)diff.p + (size_t)std::max(nk, 1) * D;
    // sparsified graph: factor, log det, Mahalanobis term || L_x^T diff ||^2
    if ((rc = so->factorise(s, gbo, bad1))) return rc;
    so->logdiag(s, 0, out, 1);
    launch_pose_diff(D, s, base.dev_arena, (const int64_t *)vb.p, other.dev_arena, (const int64_t *)vo.p, nk, dk);
    hipLaunchKernelGGL(scatter_blocks_kernel, dim3((nk * D + 255) / 256), dim3(256), 0, s, (const double *)dk, (const int32_t *)dpos.p, nk, D, dperm);
    so->ltx_norm2(s, dperm, out, 3);
    // baseline: marginalised blocks first; log det of the marginal from the kept supernodes; selected inverse
    if ((rc = sb->factorise(s, gbb, bad0))) return rc;
    sb->logdiag(s, n_marg_sn, out, 2);
    if ((rc = sb->selected_inverse(s, bad0))) return rc;
    // trace(Sigma_kept Lambda_x): the sparsified graph's Hessian blocks against the selected inverse
    const TraceSink ts{FrontSink{sb->dev, bad0}, (double *)tpart.p, 0.0};
    by_dim(D, [&](auto d) { launch_assemble_into<decltype(d)::value>(gbx, ts, s, nullptr); });
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, s, (const double *)tpart.p, other_.nv, out, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(timer.stop(s));
    int h_bad[2] = {0, 0};
    double h_out[4] = {0, 0, 0, 0};
    float ms = 0;
    HIPCHK(hipMemcpyAsync(h_out, outb.p, 4 * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_bad, bad.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(timer.ms(ms));
    if (h_bad[0] == 2) { snprintf(err, errlen, "sparse KLD: an edge of the sparsified graph lies outside the fill of the baseline's marginal"); return SPG_ESTATE; }
    if (h_bad[0] || h_bad[1]) {
        snprintf(err, errlen, "global KLD: %s information matrix is not positive definite", h_bad[0] ? "the baseline" : "the sparsified");
        return SPG_ENOTPD;
    }
    const double n_keep = (double)D * nk;
    const double innerprod = h_out[0], logdetx = 2 * h_out[1], logdety = -2 * h_out[2], mahal = h_out[3];
    terms.kld = 0.5 * (innerprod + mahal - logdetx - logdety - n_keep);
    terms.innerprod = innerprod; terms.mahalanobis = mahal; terms.logdetx = logdetx; terms.logdety = logdety; terms.n = (int64_t)n_keep;
    terms.device_seconds += 1e-3 * ms;
    return 0;
}

// Covariance blocks of a staged graph (in.pos >= 0: its free vertices, ascending = the block numbering) from the selected
// inverse over its own plan: no marginalised part, so the item lists of the top-down recurrence cover every supernode
// and the Z blocks take sum NP^2 over all of them. req: n requests of K vertex indices (-1 = zero rows and columns);
// the blocks land in d_out (device, n (K D)^2 doubles). The fronts are released on return, before a caller factorises
// a second graph. stats += supernodes, bytes of fronts and Z blocks, factorisation flops, selected-inverse flops and the
// HIP-event time of assembly, factorisation, selected inverse and extraction.
static int sigma_blocks(hipStream_t s, const DenseGraphIn &in_, int K, const int32_t *req, int n, double *d_out, spg_cov_stats &stats,
                        char *err, size_t errlen) {
    const int D = in_.D;
    int rc = 0;
    sparse::Plan plan;
    std::vector<int32_t> pos;
    plan_of(in_, nullptr, plan, pos);
    std::vector<int32_t> rpos((size_t)n * K);
    for (size_t i = 0; i < rpos.size(); i++) {
        rpos[i] = req[i] < 0 ? -1 : pos[req[i]];
        if (req[i] >= 0 && rpos[i] < 0) { snprintf(err, errlen, "covariance blocks: a requested vertex is not a variable"); return SPG_ESTATE; }
    }
    auto sp = std::make_unique<SparseSolver>();
    if ((rc = sp->init(std::move(plan), true, err, errlen))) return rc;
    sp->count_into(stats);
    DenseGraphIn in = in_;
    in.pos = pos.data();
    GraphBufs gb;
    DevBuf bad, dreq;
    HIPCHK(hipMalloc(&bad.p, 2 * sizeof(int)));
    EventTimer timer;
    if ((rc = upload(dreq, rpos.data(), rpos.size(), s)) || (rc = stage_graph(in, gb, s))) {
        snprintf(err, errlen, "staging the graph for the covariance blocks failed (%d)", rc);
        return rc;
    }
    HIPCHK(hipMemsetAsync(bad.p, 0, 2 * sizeof(int), s));
    HIPCHK(timer.start(s));
    if ((rc = sp->factorise(s, gb, (int *)bad.p))) { snprintf(err, errlen, "sparse assembly failed"); return rc; }
    if ((rc = sp->selected_inverse(s, (int *)bad.p))) { snprintf(err, errlen, "selected inverse failed"); return rc; }
    if (n > 0) {
        const FrontSink fs{sp->dev, (int *)bad.p + 1};
        const int32_t *rq = (const int32_t *)dreq.p;
        by_dim(D, [&](auto d) {
            auto launch = [&](auto k) { hipLaunchKernelGGL((sp_sigma_blocks_kernel<decltype(d)::value, decltype(k)::value>), dim3(n), dim3(64), 0, s, fs, rq, n, d_out); };
            if (K == 1) launch(std::integral_constant<int, 1>{});
            else launch(std::integral_constant<int, 2>{});
        });
    }
    HIPCHK(hipGetLastError());
    HIPCHK(timer.stop(s));
    int h_bad[2] = {0, 0};
    float ms = 0;
    HIPCHK(hipMemcpyAsync(h_bad, bad.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(timer.ms(ms));
    stats.device_seconds += 1e-3 * ms;
    return cov_bad_flags(h_bad, err, errlen);
}

int hip_sparse_cov_blocks(void *stream, const DenseGraphIn &in, int K, const int32_t *req, int n, double *out, spg_cov_stats &stats,
                          char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    const int W = K * in.D;
    const size_t len = (size_t)std::max(n, 1) * W * W;
    DevBuf dout;
    HIPCHK(hipMalloc(&dout.p, len * 8));
    if (int rc = sigma_blocks(s, in, K, req, n, (double *)dout.p, stats, err, errlen)) return rc;
    if (n > 0) HIPCHK(hipMemcpy(out, dout.p, (size_t)n * W * W * 8, hipMemcpyDeviceToHost));
    return 0;
}

// Covariance sub-blocks of arbitrary vertex pairs (spg_graph_pair_covariances / _joint_marginal_covariance). Sub-block i
// is Sigma(va[i], vb[i]) (D x D, -1 = the fixed vertex: zero) at out + dst[i], row stride ld. Diagonal and in-pattern
// sub-blocks are read from the selected inverse (bit for bit what sigma_blocks reads; SPG_COV_FORCE_SOLVE=1 sends them
// through the solves as well); the others take one column solve per pair of vertices, shared by (a, b) and (b, a).
// Order on the device: factorisation, column solves on the intact factor, selected inverse, one assembly launch.
// cov_solve_device leaves the assembled sub-blocks in dout (device, out_len doubles); `tail`, if given, launches what
// consumes them there (it sees the staged graph; its launches are inside the selected inverse's event pair) before the
// fronts are released. hip_sparse_cov_solve adds the copy to the host.
// `post`, if given, runs last, after the synchronisation and the checks, while the solver and the staged graph are
// still alive (the lazy greedy rounds): it gets the solver, whose fronts then hold the selected inverse, the staged graph,
// the device flags and pos (per vertex index: D * elimination position).
using CovTail = std::function<void(hipStream_t, const GraphBufs &, const double *)>;
using CovPost = std::function<int(hipStream_t, SparseSolver &, const GraphBufs &, int *, const std::vector<int32_t> &)>;
static int cov_solve_device(hipStream_t s, const DenseGraphIn &in_, const int32_t *va, const int32_t *vb, const int64_t *dst, int32_t ld, int64_t nblk,
                            int64_t out_len, DevBuf &dout, spg_cov_solve_stats &stats, char *err, size_t errlen, const CovTail *tail,
                            const CovPost *post = nullptr) {
    const int D = in_.D;
    const bool force = cov_force_solve();
    int rc = 0;
    sparse::Plan plan;
    std::vector<int32_t> pos;
    plan_of(in_, nullptr, plan, pos);
    for (int64_t i = 0; i < nblk; i++)
        if ((va[i] >= 0 && pos[va[i]] < 0) || (vb[i] >= 0 && pos[vb[i]] < 0)) {
            snprintf(err, errlen, "covariance blocks: a requested vertex is not a variable");
            return SPG_ESTATE;
        }
    auto sp = std::make_unique<SparseSolver>();
    if ((rc = sp->init(std::move(plan), true, err, errlen))) return rc;
    const Plan &P = sp->plan;
    // sub-blocks -> selected inverse or a cross block; one cross block per unordered pair of positions
    std::vector<CovBlk> blks((size_t)nblk);
    std::vector<int32_t> cx, cy;    // cross requests: block positions x <= y
    {
        std::unordered_map<uint64_t, int32_t> key;
        for (int64_t i = 0; i < nblk; i++) {
            CovBlk &b = blks[i];
            b = CovBlk{dst[i], ld, va[i] < 0 ? -1 : pos[va[i]], vb[i] < 0 ? -1 : pos[vb[i]], -1, 0, 0};
            if (b.pa < 0 || b.pb < 0) { b.pa = b.pb = -1; continue; }
            const int qa = b.pa / D, qb = b.pb / D;
            if (!force && (qa == qb || in_fronts(P, qa, qb))) continue;
            const int x = std::min(qa, qb), y = std::max(qa, qb);
            auto it = key.emplace(((uint64_t)x << 32) | (uint32_t)y, (int32_t)cx.size());
            if (it.second) { cx.push_back(x); cy.push_back(y); }
            b.cross = it.first->second;
        }
    }
    std::vector<int32_t> ccol, crow(cx.size());
    choose_columns(P.n, cx, cy, ccol);
    for (size_t i = 0; i < cx.size(); i++) crow[i] = ccol[i] == cx[i] ? cy[i] : cx[i];
    for (CovBlk &b : blks)   // the cross block holds Sigma(row, column): transposed when a is the solved column
        if (b.cross >= 0) b.tr = (b.pa / D == ccol[b.cross] && b.pa != b.pb) ? 1 : 0;
    ColumnSolves cs(*sp, crow, ccol);
    DenseGraphIn in = in_;
    in.pos = pos.data();
    GraphBufs gb;
    DevBuf bad, dcross, dblk;
    int h_bad[2] = {0, 0};
    float ms0 = 0, ms1 = 0;
    HIPCHK(hipMalloc(&bad.p, 2 * sizeof(int)));
    HIPCHK(hipMalloc(&dout.p, (size_t)std::max<int64_t>(out_len, 1) * 8));
    HIPCHK(hipMalloc(&dcross.p, std::max<size_t>(cx.size(), 1) * D * D * 8));
    EventTimer t_factor, t_selinv;   // the column solves in between keep their own time (ColumnSolves::seconds)
    if ((rc = upload(dblk, blks.data(), blks.size(), s)) || (rc = stage_graph(in, gb, s))) {
        snprintf(err, errlen, "staging the graph for the covariance blocks failed (%d)", rc);
        return rc;
    }
    HIPCHK(hipMemsetAsync(bad.p, 0, 2 * sizeof(int), s));
    HIPCHK(t_factor.start(s));
    if ((rc = sp->factorise(s, gb, (int *)bad.p))) { snprintf(err, errlen, "sparse assembly failed"); return rc; }
    HIPCHK(t_factor.stop(s));
    HIPCHK(hipMemcpyAsync(h_bad, bad.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h_bad[0]) return cov_bad_flags(h_bad, err, errlen);
    HIPCHK(t_factor.ms(ms0));
    if ((rc = cs.run(s, (double *)dcross.p, err, errlen))) return rc;
    HIPCHK(t_selinv.start(s));
    if ((rc = sp->selected_inverse(s, (int *)bad.p))) { snprintf(err, errlen, "selected inverse failed"); return rc; }
    if (nblk > 0) {
        const FrontSink fs{sp->dev, (int *)bad.p + 1};
        by_dim(D, [&](auto d) {
            hipLaunchKernelGGL((sp_cov_assemble_kernel<decltype(d)::value>), dim3((unsigned)((nblk + 3) / 4)), dim3(256), 0, s, fs, (const CovBlk *)dblk.p, (int)nblk,
                               (const double *)dcross.p, (double *)dout.p);
        });
    }
    if (tail) (*tail)(s, gb, (const double *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(t_selinv.stop(s));
    HIPCHK(hipMemcpyAsync(h_bad, bad.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(t_selinv.ms(ms1));
    if ((rc = cov_bad_flags(h_bad, err, errlen))) return rc;
    sp->count_into(stats.cov);
    stats.cov.device_seconds += 1e-3 * (ms0 + ms1) + cs.seconds;
    stats.columns += (int32_t)cs.cols.size(); stats.rhs_batches += cs.nbatch; stats.solve_flops += cs.flops; stats.solve_seconds += cs.seconds;
    if (post) return (*post)(s, *sp, gb, (int *)bad.p, pos);
    return 0;
}

int hip_sparse_cov_solve(void *stream, const DenseGraphIn &in, const int32_t *va, const int32_t *vb, const int64_t *dst, int32_t ld, int64_t nblk,
                         int64_t out_len, double *out, spg_cov_solve_stats &stats, char *err, size_t errlen) {
    DevBuf dout;
    if (int rc = cov_solve_device((hipStream_t)stream, in, va, vb, dst, ld, nblk, out_len, dout, stats, err, errlen, nullptr)) return rc;
    if (out_len > 0) HIPCHK(hipMemcpy(out, dout.p, (size_t)out_len * 8, hipMemcpyDeviceToHost));
    return 0;
}

// spg_graph_relative_covariances (rec == nullptr: rel, may be nullptr, and cov) and spg_graph_score_candidates (rec: n
// records; d2 / gain / chi2 / status, each may be nullptr). The sub-block lists describe one 2D x 2D block per distinct
// pair (cov_solve_device); candidate i reads block slot[i] and the poses of vertex indices ca[i], cb[i]. Only the
// results cross to the host.
int hip_sparse_relative(void *stream, const DenseGraphIn &in, const int32_t *va, const int32_t *vb, const int64_t *dst, int32_t ld, int64_t nblk,
                        int64_t blocks_len, const int32_t *ca, const int32_t *cb, const int32_t *slot, int n, const double *rec, double *rel,
                        double *cov, double *d2, double *gain, double *chi2, int32_t *status, spg_cov_solve_stats &stats, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    const int D = in.D, PS = D == 6 ? 7 : 3, REC = PS + D * (D + 1) / 2;
    const size_t nn = (size_t)std::max(n, 1);
    int rc = 0;
    DevBuf dblocks, dca, dcb, dslot, drec, drel, dcov, dscore, dstatus;
    if ((rc = upload(dca, ca, (size_t)n, s)) || (rc = upload(dcb, cb, (size_t)n, s)) || (rc = upload(dslot, slot, (size_t)n, s)) ||
        (rec && (rc = upload(drec, rec, (size_t)n * REC, s)))) {
        snprintf(err, errlen, "staging the candidates failed (%d)", rc);
        return rc;
    }
    if (rec) {
        HIPCHK(hipMalloc(&dscore.p, nn * 3 * 8));
        HIPCHK(hipMalloc(&dstatus.p, nn * sizeof(int32_t)));
    } else {
        HIPCHK(hipMalloc(&drel.p, nn * PS * 8));
        HIPCHK(hipMalloc(&dcov.p, nn * D * D * 8));
    }
    const CovTail tail = [&](hipStream_t st, const GraphBufs &gb, const double *blocks) {
        if (n <= 0) return;
        const RelArgs ra{gb.dev.arena, gb.dev.vpo, (const int32_t *)dca.p, (const int32_t *)dcb.p, (const int32_t *)dslot.p, (const double *)drec.p, blocks,
                         (double *)drel.p, (double *)dcov.p, (double *)dscore.p, (int32_t *)dstatus.p, n};
        by_dim(D, [&](auto d) { hipLaunchKernelGGL((sp_relative_kernel<decltype(d)::value>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, ra); });
    };
    if ((rc = cov_solve_device(s, in, va, vb, dst, ld, nblk, blocks_len, dblocks, stats, err, errlen, &tail))) return rc;
    if (n <= 0) return 0;
    if (rec) {
        const double *sc = (const double *)dscore.p;
        if (d2) HIPCHK(hipMemcpy(d2, sc, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (gain) HIPCHK(hipMemcpy(gain, sc + n, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (chi2) HIPCHK(hipMemcpy(chi2, sc + 2 * (size_t)n, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (status) HIPCHK(hipMemcpy(status, dstatus.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    } else {
        if (rel) HIPCHK(hipMemcpy(rel, drel.p, (size_t)n * PS * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cov, dcov.p, (size_t)n * D * D * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

// ---- the two greedy calls and their lazy mode (SPG_GREEDY_LAZY, DESIGN 5g-L)
constexpr int kGreedyCtl = 4 + 16;   // control words, then the ranked list (at most 64 / 2D = 10 candidates)

// by_dim with the LAZY / RANK flag of the greedy kernels as a second compile-time constant: f(d, std::true_type) or false
template <class F>
void by_dim_lazy(int D, bool lazy, F &&f) {
    by_dim(D, [&](auto d) { lazy ? f(d, std::true_type{}) : f(d, std::false_type{}); });
}

// by_dim_lazy with the objective of the edge kernels (OBJ_LOSS / OBJ_STAT) as a third constant
template <class F>
void by_dim_lazy_obj(int D, bool lazy, int obj, F &&f) {
    by_dim_lazy(D, lazy, [&](auto d, auto lz) {
        obj == OBJ_STAT ? f(d, lz, std::integral_constant<int, OBJ_STAT>{}) : f(d, lz, std::integral_constant<int, OBJ_LOSS>{});
    });
}

// The free-HBM check of a greedy call, before anything is allocated. bytes: the joint block (a lazy call: the pair
// blocks), blocks_len doubles, plus the histories and the state; a lazy call adds two column strips, and its panel
// workspace is checked once the plan is known.
static int greedy_capacity(const char *what, double bytes, int64_t blocks_len, int D, const GreedyLazyIn *lazy, char *err, size_t errlen) {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const double strips = lazy ? 2.0 * 8.0 * (double)lazy->m * D * D : 0.0;
    if (bytes + strips + (double)(1ull << 30) <= (double)free_b) return 0;
    if (lazy)
        snprintf(err, errlen, "%s (lazy) needs %.2f GB of pair blocks, %.2f GB of histories and state and %.2f GB for two column strips, %.1f GB are free",
                 what, blocks_len * 8e-9, (bytes - 8.0 * (double)blocks_len) * 1e-9, strips * 1e-9, free_b * 1e-9);
    else
        snprintf(err, errlen, "%s needs %.1f GB for the joint covariance of the endpoints and the histories, %.1f GB are free", what, bytes * 1e-9,
                 free_b * 1e-9);
    return SPG_ECAPACITY;
}

// The rounds of a lazy call, after round 0 (init kernel, in the selected inverse's event pair) has been synchronised: the
// factor is rebuilt (the selected inverse overwrote it), then per round: pick() = argmax / argmin stage 1 and the
// ranking stage 2; the host reads the control words and the ranked list (one synchronisation), stops on the device's stop word,
// lets the planner choose the columns to solve, sweeps them into their strips and launches round() with the strips of
// a*, b* in z. gather() and the call's timer end the device part.
template <class Pick, class Round, class Gather>
static int greedy_lazy_rounds(hipStream_t st, SparseSolver &sp, const GraphBufs &gb, int *bad, const std::vector<int32_t> &pos, const GreedyLazyIn &lz, int look,
                              const int32_t *sa, const int32_t *sb, int kk, int32_t *dctl, LazyArgs &z, EventTimer &t_call, spg_cov_solve_stats &cstats,
                              char *err, size_t errlen, Pick pick, Round round, Gather gather) {
    const int D = sp.D;
    std::vector<int32_t> q((size_t)lz.m);
    for (int j = 0; j < lz.m; j++) q[j] = pos[lz.S[j]] / D;
    LazySweeps sw(sp, std::move(q));
    if (int rc = sw.init(0.0, (long long)kk * (kGreedyPanel / D), err, errlen)) return rc;
    z.cache = (const double *)sw.cache.p;
    z.strip_len = sw.strip_len;
    EventTimer t_post;
    HIPCHK(t_post.start(st));
    if (int rc = sp.factorise(st, gb, bad)) { snprintf(err, errlen, "sparse assembly failed"); return rc; }
    GreedyColumnCache cache(lz.m, sw.nstrips, kGreedyPanel / D, look);
    GreedyRound gr;
    int32_t h[kGreedyCtl];
    int rounds = 0;
    for (int t = 0; t < kk; t++) {
        pick();
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h, dctl, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (int rc = sw.collect(err, errlen)) return rc;
        if (h[1]) break;
        if (h[4] < 0 || h[4] != h[2]) { snprintf(err, errlen, "lazy greedy rounds: the ranked list does not start with the chosen candidate"); return SPG_ESTATE; }
        cache.plan(h + 4, look, sa, sb, gr);
        if (int rc = sw.solve(st, gr, err, errlen)) return rc;
        z.ca = gr.strip_a; z.cb = gr.strip_b;
        round();
        rounds++;
    }
    gather();
    HIPCHK(hipGetLastError());
    HIPCHK(t_call.stop(st));
    HIPCHK(t_post.stop(st));
    int h_bad[2] = {0, 0};
    float ms = 0;
    HIPCHK(hipMemcpyAsync(h_bad, bad, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (int rc = sw.collect(err, errlen)) return rc;
    if (int rc = cov_bad_flags(h_bad, err, errlen)) return rc;
    HIPCHK(t_post.ms(ms));
    cstats.cov.device_seconds += 1e-3 * ms;
    if (lz.stats) {
        spg_greedy_stats &gs = *lz.stats;
        gs = spg_greedy_stats{};
        gs.method = SPG_GREEDY_LAZY; gs.lookahead = look; gs.rounds = rounds; gs.refactorised = 1;
        gs.column_vertices = cache.column_vertices; gs.column_hits = cache.column_hits;
        gs.rhs_batches = sw.batches; gs.evictions = (int32_t)cache.evictions;
        gs.round_solve_seconds = sw.cs.seconds; gs.cache_bytes = sw.cache_bytes();
    }
    return 0;
}

// spg_graph_select_candidates: the sub-block lists describe the m D x m D joint covariance of the candidates' endpoints
// (joint_len doubles, row stride ld, kept on the device); candidate i has the poses of vertex indices ca[i], cb[i] and
// the endpoint slots sa[i], sb[i] (-1: the fixed vertex). The tail enqueues init, kk x (argmax, pick, round) and the
// gather without a synchronisation; the stop rules are device words the later launches return on. selected / cond_gain:
// kk entries (the tail beyond *nsel is -1 / NaN), final_gain / status: n each, may be nullptr. Host arrays throughout.
int hip_sparse_select(void *stream, const DenseGraphIn &in, const int32_t *va, const int32_t *vb, const int64_t *dst, int32_t ld, int64_t nblk,
                      int64_t joint_len, const int32_t *ca, const int32_t *cb, const int32_t *sa, const int32_t *sb, int n, const double *rec, int kk,
                      double min_gain, double max_d2, int32_t *selected, double *cond_gain, double *final_gain, int32_t *status, int *nsel,
                      spg_select_stats &stats, char *err, size_t errlen, const GreedyLazyIn *lazy) {
    hipStream_t s = (hipStream_t)stream;
    const int D = in.D, DD = D * D, PS = D == 6 ? 7 : 3, REC = PS + D * (D + 1) / 2;
    const int np = std::min((n + 255) / 256, 256);
    const int look = lazy ? greedy_lookahead(lazy->lookahead, D) : 0;
    const double bytes = 8.0 * ((double)joint_len + (double)n * kk * DD + (double)n * (4 * DD + 3));
    int rc = 0;
    if ((rc = greedy_capacity("candidate selection", bytes, joint_len, D, lazy, err, errlen))) return rc;
    DevBuf djoint, dca, dcb, dsa, dsb, drec, dJ, dL, dC, dhist, dgain, dd2, dstate, dpg, dpi, dctl, dpub, dsel, dcg, dfinal, dpslot;
    if ((rc = upload(dca, ca, (size_t)n, s)) || (rc = upload(dcb, cb, (size_t)n, s)) || (rc = upload(dsa, sa, (size_t)n, s)) ||
        (rc = upload(dsb, sb, (size_t)n, s)) || (rc = upload(drec, rec, (size_t)n * REC, s)) || (lazy && (rc = upload(dpslot, lazy->pslot, (size_t)n, s)))) {
        snprintf(err, errlen, "staging the candidates failed (%d)", rc);
        return rc;
    }
    HIPCHK(hipMalloc(&dJ.p, (size_t)n * 2 * DD * 8));
    HIPCHK(hipMalloc(&dL.p, (size_t)n * DD * 8));
    HIPCHK(hipMalloc(&dC.p, (size_t)n * DD * 8));
    HIPCHK(hipMalloc(&dhist.p, (size_t)n * kk * DD * 8));
    HIPCHK(hipMalloc(&dgain.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&dd2.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&dstate.p, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dpg.p, (size_t)np * 8));
    HIPCHK(hipMalloc(&dpi.p, (size_t)np * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dctl.p, kGreedyCtl * sizeof(int32_t)));   // 4 control words, then the lazy form's ranked list
    HIPCHK(hipMalloc(&dpub.p, (size_t)DD * 8));
    HIPCHK(hipMalloc(&dsel.p, (size_t)kk * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dcg.p, (size_t)kk * 8));
    HIPCHK(hipMalloc(&dfinal.p, (size_t)n * 8));
    HIPCHK(hipMemsetAsync(dctl.p, 0, 4 * sizeof(int32_t), s));
    HIPCHK(hipMemsetAsync(dsel.p, 0xff, (size_t)kk * sizeof(int32_t), s));   // -1
    HIPCHK(hipMemsetAsync(dcg.p, 0xff, (size_t)kk * 8, s));                  // NaN
    EventTimer t_select;
    hipError_t tail_err = hipSuccess;
    SelArgs a{};
    LazyArgs z{};
    // the launches of the call, on s (the stream tail and post are handed), once tail has filled a and z
    const dim3 per_cand((unsigned)((n + 3) / 4)), wg(256);
    const auto init = [&] {
        by_dim_lazy(D, lazy, [&](auto d, auto lz) {
            hipLaunchKernelGGL((sp_select_init_kernel<decltype(d)::value, decltype(lz)::value>), per_cand, wg, 0, s, a, z);
        });
    };
    const auto stage1 = [&] { hipLaunchKernelGGL(sp_select_argmax_kernel, dim3((unsigned)np), wg, 0, s, a); };
    const auto stage2 = [&] {
        by_dim_lazy(D, lazy, [&](auto d, auto lz) {
            hipLaunchKernelGGL((sp_select_pick_kernel<decltype(d)::value, decltype(lz)::value>), dim3(1), wg, 0, s, a, z);
        });
    };
    const auto round = [&] {
        by_dim_lazy(D, lazy, [&](auto d, auto lz) {
            hipLaunchKernelGGL((sp_select_round_kernel<decltype(d)::value, decltype(lz)::value>), per_cand, wg, 0, s, a, z);
        });
    };
    const auto gather = [&] { hipLaunchKernelGGL(sp_select_gather_kernel, dim3((unsigned)((n + 255) / 256)), wg, 0, s, a); };
    const CovTail tail = [&](hipStream_t st, const GraphBufs &gb, const double *joint) {
        a.arena = gb.dev.arena; a.vpo = gb.dev.vpo;
        a.va = (const int32_t *)dca.p; a.vb = (const int32_t *)dcb.p; a.sa = (const int32_t *)dsa.p; a.sb = (const int32_t *)dsb.p;
        a.rec = (const double *)drec.p; a.joint = joint; a.ld = ld;
        a.J = (double *)dJ.p; a.L = (double *)dL.p; a.C = (double *)dC.p; a.hist = (double *)dhist.p;
        a.gain = (double *)dgain.p; a.d2 = (double *)dd2.p; a.state = (int32_t *)dstate.p;
        a.pg = (double *)dpg.p; a.pi = (int32_t *)dpi.p; a.ctl = (int32_t *)dctl.p; a.pubC = (double *)dpub.p;
        a.sel = (int32_t *)dsel.p; a.cg = (double *)dcg.p; a.final_gain = (double *)dfinal.p;
        a.n = n; a.kk = kk; a.np = np; a.min_gain = min_gain; a.max_d2 = max_d2;
        if (lazy) {   // round 0 from the pair blocks; the rounds follow in `post`, on the factor
            a.joint = nullptr; a.ld = 0;
            z.blocks = joint; z.pslot = (const int32_t *)dpslot.p; z.rank = (int32_t *)dctl.p + 4; z.L = look; z.ca = z.cb = -1;
        }
        tail_err = t_select.start(st);
        init();
        if (lazy) return;
        for (int t = 0; t < kk; t++) { stage1(); stage2(); round(); }
        gather();
        if (tail_err == hipSuccess) tail_err = t_select.stop(st);
    };
    const CovPost post = [&](hipStream_t st, SparseSolver &sp, const GraphBufs &gb, int *bad, const std::vector<int32_t> &pos) -> int {
        return greedy_lazy_rounds(st, sp, gb, bad, pos, *lazy, look, sa, sb, kk, (int32_t *)dctl.p, z, t_select, stats.solve, err, errlen,
                                  [&] { stage1(); stage2(); }, round, gather);
    };
    if ((rc = cov_solve_device(s, in, va, vb, dst, ld, nblk, joint_len, djoint, stats.solve, err, errlen, &tail, lazy ? &post : nullptr))) return rc;
    HIPCHK(tail_err);
    float ms = 0;
    HIPCHK(t_select.ms(ms));
    int32_t ctl[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(ctl, dctl.p, sizeof ctl, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(selected, dsel.p, (size_t)kk * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cond_gain, dcg.p, (size_t)kk * 8, hipMemcpyDeviceToHost));
    if (final_gain) HIPCHK(hipMemcpy(final_gain, dfinal.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, dstate.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    *nsel = ctl[0];
    stats.rounds = ctl[0];
    stats.select_seconds = 1e-3 * ms;
    return 0;
}

// spg_graph_prune_candidates (obj = OBJ_LOSS) and spg_graph_detect_outliers (OBJ_STAT): the sub-block lists and slots as
// hip_sparse_select; candidate i is live edge eidx[i] of the staged graph. The tail enqueues init, kk x (argmin / argmax,
// pick, round) and the gather without a synchronisation. chosen / value / kld: kk entries (the tail beyond *nchosen is
// -1 / NaN; kld: OBJ_LOSS only), final_value / final_margin / status: n each, may be nullptr; redundancy (OBJ_STAT, n,
// may be nullptr) = D - tr0. limit: max_loss or min_stat. Host arrays throughout.
struct EdgeGreedyTimes { spg_cov_solve_stats &solve; int32_t &rounds; double &seconds; };
static int greedy_edges(int obj, const char *what, void *stream, const DenseGraphIn &in, const int32_t *va, const int32_t *vb, const int64_t *dst, int32_t ld,
                        int64_t nblk, int64_t joint_len, const int32_t *eidx, const int32_t *sa, const int32_t *sb, int n, int kk, double limit,
                        double max_kld, double min_margin, int32_t *pruned, double *cond_loss, double *kld, double *final_loss, double *final_margin,
                        double *redundancy, int32_t *status, int *npruned, EdgeGreedyTimes stats, char *err, size_t errlen, const GreedyLazyIn *lazy) {
    hipStream_t s = (hipStream_t)stream;
    const int D = in.D, DD = D * D;
    const bool snoop = obj == OBJ_STAT;
    const int np = std::min((n + 255) / 256, 256);
    const int look = lazy ? greedy_lookahead(lazy->lookahead, D) : 0;
    const double bytes = 8.0 * ((double)joint_len + (double)n * kk * DD + (double)n * (4 * DD + 7 + (snoop ? D : 0)));
    int rc = 0;
    if ((rc = greedy_capacity(what, bytes, joint_len, D, lazy, err, errlen))) return rc;
    DevBuf djoint, deidx, dsa, dsb, dJ, dL, dC, dhist, dloss, dmargin, dtr0, dstate, dpg, dpi, dctl, dpub, dksum, dsel, dcl, dck, dfl, dfm, dstatus, dpslot, de;
    if ((rc = upload(deidx, eidx, (size_t)n, s)) || (rc = upload(dsa, sa, (size_t)n, s)) || (rc = upload(dsb, sb, (size_t)n, s)) ||
        (lazy && (rc = upload(dpslot, lazy->pslot, (size_t)n, s)))) {
        snprintf(err, errlen, "staging the candidates failed (%d)", rc);
        return rc;
    }
    HIPCHK(hipMalloc(&dJ.p, (size_t)n * 2 * DD * 8));
    HIPCHK(hipMalloc(&dL.p, (size_t)n * DD * 8));
    HIPCHK(hipMalloc(&dC.p, (size_t)n * DD * 8));
    HIPCHK(hipMalloc(&dhist.p, (size_t)n * kk * DD * 8));
    HIPCHK(hipMalloc(&dloss.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&dmargin.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&dtr0.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&dstate.p, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dpg.p, (size_t)np * 8));
    HIPCHK(hipMalloc(&dpi.p, (size_t)np * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dctl.p, kGreedyCtl * sizeof(int32_t)));   // 4 control words, then the lazy form's ranked list
    HIPCHK(hipMalloc(&dpub.p, (size_t)(DD + (snoop ? D : 0)) * 8));
    if (snoop) HIPCHK(hipMalloc(&de.p, (size_t)n * D * 8));
    if (!snoop) HIPCHK(hipMalloc(&dksum.p, 8));
    HIPCHK(hipMalloc(&dsel.p, (size_t)kk * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dcl.p, (size_t)kk * 8));
    if (!snoop) HIPCHK(hipMalloc(&dck.p, (size_t)kk * 8));   // the statistic has no KLD: cl alone
    HIPCHK(hipMalloc(&dfl.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&dfm.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&dstatus.p, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMemsetAsync(dctl.p, 0, 4 * sizeof(int32_t), s));
    if (!snoop) HIPCHK(hipMemsetAsync(dksum.p, 0, 8, s));
    HIPCHK(hipMemsetAsync(dsel.p, 0xff, (size_t)kk * sizeof(int32_t), s));   // -1
    HIPCHK(hipMemsetAsync(dcl.p, 0xff, (size_t)kk * 8, s));                  // NaN
    if (!snoop) HIPCHK(hipMemsetAsync(dck.p, 0xff, (size_t)kk * 8, s));
    EventTimer t_prune;
    hipError_t tail_err = hipSuccess;
    PruneArgs a{};
    LazyArgs z{};
    // the launches of the call, on s (the stream tail and post are handed), once tail has filled a and z
    const dim3 per_cand((unsigned)((n + 3) / 4)), wg(256);
    const auto init = [&] {
        by_dim_lazy_obj(D, lazy, obj, [&](auto d, auto lz, auto o) {
            hipLaunchKernelGGL((sp_prune_init_kernel<decltype(d)::value, decltype(lz)::value, decltype(o)::value>), per_cand, wg, 0, s, a, z);
        });
    };
    const auto stage1 = [&] {
        if (snoop) hipLaunchKernelGGL(sp_prune_argmin_kernel<OBJ_STAT>, dim3((unsigned)np), wg, 0, s, a);
        else hipLaunchKernelGGL(sp_prune_argmin_kernel<OBJ_LOSS>, dim3((unsigned)np), wg, 0, s, a);
    };
    const auto stage2 = [&] {
        by_dim_lazy_obj(D, lazy, obj, [&](auto d, auto lz, auto o) {
            hipLaunchKernelGGL((sp_prune_pick_kernel<decltype(d)::value, decltype(lz)::value, decltype(o)::value>), dim3(1), wg, 0, s, a, z);
        });
    };
    const auto round = [&] {
        by_dim_lazy_obj(D, lazy, obj, [&](auto d, auto lz, auto o) {
            hipLaunchKernelGGL((sp_prune_round_kernel<decltype(d)::value, decltype(lz)::value, decltype(o)::value>), per_cand, wg, 0, s, a, z);
        });
    };
    const auto gather = [&] { hipLaunchKernelGGL(sp_prune_gather_kernel, dim3((unsigned)((n + 255) / 256)), wg, 0, s, a); };
    const CovTail tail = [&](hipStream_t st, const GraphBufs &gb, const double *joint) {
        a.arena = gb.dev.arena; a.vpo = gb.dev.vpo; a.er = gb.dev.er; a.ev = gb.dev.ev;
        a.eidx = (const int32_t *)deidx.p; a.sa = (const int32_t *)dsa.p; a.sb = (const int32_t *)dsb.p;
        a.joint = joint; a.ld = ld;
        a.J = (double *)dJ.p; a.L = (double *)dL.p; a.C = (double *)dC.p; a.hist = (double *)dhist.p;
        a.loss = (double *)dloss.p; a.margin = (double *)dmargin.p; a.tr0 = (double *)dtr0.p; a.state = (int32_t *)dstate.p;
        a.pg = (double *)dpg.p; a.pi = (int32_t *)dpi.p; a.ctl = (int32_t *)dctl.p; a.pubC = (double *)dpub.p;
        if (snoop) a.e = (double *)de.p;
        else a.kldsum = (double *)dksum.p;
        a.sel = (int32_t *)dsel.p; a.cl = (double *)dcl.p; a.ck = (double *)dck.p;
        a.final_loss = (double *)dfl.p; a.final_margin = (double *)dfm.p; a.status = (int32_t *)dstatus.p;
        a.n = n; a.kk = kk; a.np = np; a.max_kld = max_kld; a.min_margin = min_margin;
        if (snoop) a.min_stat = limit;
        else a.max_loss = limit;
        if (lazy) {   // round 0 from the pair blocks; the rounds follow in `post`, on the factor
            a.joint = nullptr; a.ld = 0;
            z.blocks = joint; z.pslot = (const int32_t *)dpslot.p; z.rank = (int32_t *)dctl.p + 4; z.L = look; z.ca = z.cb = -1;
        }
        tail_err = t_prune.start(st);
        init();
        if (lazy) return;
        for (int t = 0; t < kk; t++) { stage1(); stage2(); round(); }
        gather();
        if (tail_err == hipSuccess) tail_err = t_prune.stop(st);
    };
    const CovPost post = [&](hipStream_t st, SparseSolver &sp, const GraphBufs &gb, int *bad, const std::vector<int32_t> &pos) -> int {
        return greedy_lazy_rounds(st, sp, gb, bad, pos, *lazy, look, sa, sb, kk, (int32_t *)dctl.p, z, t_prune, stats.solve, err, errlen,
                                  [&] { stage1(); stage2(); }, round, gather);
    };
    if ((rc = cov_solve_device(s, in, va, vb, dst, ld, nblk, joint_len, djoint, stats.solve, err, errlen, &tail, lazy ? &post : nullptr))) return rc;
    HIPCHK(tail_err);
    float ms = 0;
    HIPCHK(t_prune.ms(ms));
    int32_t ctl[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(ctl, dctl.p, sizeof ctl, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pruned, dsel.p, (size_t)kk * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cond_loss, dcl.p, (size_t)kk * 8, hipMemcpyDeviceToHost));
    if (kld) HIPCHK(hipMemcpy(kld, dck.p, (size_t)kk * 8, hipMemcpyDeviceToHost));
    if (redundancy) {   // D - tr(L_i^T C_ii(0) L_i); NaN where Omega is not PD
        HIPCHK(hipMemcpy(redundancy, dtr0.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) redundancy[i] = (double)D - redundancy[i];
    }
    if (final_loss) HIPCHK(hipMemcpy(final_loss, dfl.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (final_margin) HIPCHK(hipMemcpy(final_margin, dfm.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, dstatus.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    *npruned = ctl[0];
    stats.rounds = ctl[0];
    stats.seconds = 1e-3 * ms;
    return 0;
}

int hip_sparse_prune(void *stream, const DenseGraphIn &in, const int32_t *va, const int32_t *vb, const int64_t *dst, int32_t ld, int64_t nblk,
                     int64_t joint_len, const int32_t *eidx, const int32_t *sa, const int32_t *sb, int n, int kk, double max_loss, double max_kld,
                     double min_margin, int32_t *pruned, double *cond_loss, double *kld, double *final_loss, double *final_margin, int32_t *status,
                     int *npruned, spg_prune_stats &stats, char *err, size_t errlen, const GreedyLazyIn *lazy) {
    return greedy_edges(OBJ_LOSS, "edge pruning", stream, in, va, vb, dst, ld, nblk, joint_len, eidx, sa, sb, n, kk, max_loss, max_kld, min_margin, pruned,
                        cond_loss, kld, final_loss, final_margin, nullptr, status, npruned, {stats.solve, stats.rounds, stats.prune_seconds}, err, errlen, lazy);
}

// spg_graph_detect_outliers: flagged / stat: kk entries; final_stat, final_margin, redundancy, status: n each, may be nullptr
int hip_sparse_detect(void *stream, const DenseGraphIn &in, const int32_t *va, const int32_t *vb, const int64_t *dst, int32_t ld, int64_t nblk,
                      int64_t joint_len, const int32_t *eidx, const int32_t *sa, const int32_t *sb, int n, int kk, double min_stat, double min_margin,
                      int32_t *flagged, double *stat, double *final_stat, double *final_margin, double *redundancy, int32_t *status, int *nflagged,
                      spg_outlier_stats &stats, char *err, size_t errlen, const GreedyLazyIn *lazy) {
    return greedy_edges(OBJ_STAT, "outlier detection", stream, in, va, vb, dst, ld, nblk, joint_len, eidx, sa, sb, n, kk, min_stat, 0.0, min_margin, flagged,
                        stat, nullptr, final_stat, final_margin, redundancy, status, nflagged, {stats.solve, stats.rounds, stats.detect_seconds}, err, errlen,
                        lazy);
}

int hip_sparse_marginal_kld(void *stream, const DenseGraphIn &base, const DenseGraphIn &other, const int32_t *vb, const int32_t *vo, int nk,
                            const int64_t *vpo_base, const int64_t *vpo_other, double *kld, spg_cov_stats &stats, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    const int D = base.D;
    const size_t len = (size_t)std::max(nk, 1) * D * D;
    int rc = 0;
    DevBuf sy, sx, diff, dk, bad, pb, po;
    HIPCHK(hipMalloc(&sy.p, len * 8));
    HIPCHK(hipMalloc(&sx.p, len * 8));
    HIPCHK(hipMalloc(&diff.p, (size_t)std::max(nk, 1) * D * 8));
    HIPCHK(hipMalloc(&dk.p, (size_t)std::max(nk, 1) * 8));
    HIPCHK(hipMalloc(&bad.p, 2 * sizeof(int)));
    EventTimer timer;
    // one graph after the other: the baseline's fronts are gone before the sparsified graph is factorised
    if ((rc = sigma_blocks(s, base, 1, vb, nk, (double *)sy.p, stats, err, errlen))) {
        if (rc == SPG_ENOTPD) snprintf(err, errlen, "marginal KLD: the baseline information matrix is not positive definite");
        return rc;
    }
    if ((rc = sigma_blocks(s, other, 1, vo, nk, (double *)sx.p, stats, err, errlen))) {
        if (rc == SPG_ENOTPD) snprintf(err, errlen, "marginal KLD: the sparsified information matrix is not positive definite");
        return rc;
    }
    if ((rc = upload(pb, vpo_base, (size_t)nk, s)) || (rc = upload(po, vpo_other, (size_t)nk, s))) {
        snprintf(err, errlen, "staging the pose offsets for the marginal KLD failed (%d)", rc);
        return rc;
    }
    HIPCHK(hipMemsetAsync(bad.p, 0, 2 * sizeof(int), s));
    HIPCHK(timer.start(s));
    if (nk > 0) {
        launch_pose_diff(D, s, base.dev_arena, (const int64_t *)pb.p, other.dev_arena, (const int64_t *)po.p, nk, (double *)diff.p);
        by_dim(D, [&](auto d) {
            hipLaunchKernelGGL((sp_marginal_kld_kernel<decltype(d)::value>), dim3((nk + 63) / 64), dim3(64), 0, s, (const double *)sx.p, (const double *)sy.p, (const double *)diff.p, nk,
                               (double *)dk.p, (int *)bad.p);
        });
    }
    HIPCHK(hipGetLastError());
    HIPCHK(timer.stop(s));
    int h_bad[2] = {0, 0};
    float ms = 0;
    HIPCHK(hipMemcpyAsync(h_bad, bad.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    if (nk > 0) HIPCHK(hipMemcpyAsync(kld, dk.p, (size_t)nk * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(timer.ms(ms));
    stats.device_seconds += 1e-3 * ms;
    if (h_bad[0] || h_bad[1]) {
        snprintf(err, errlen, "marginal KLD: a marginal covariance of the %s graph is not positive definite", h_bad[0] ? "baseline" : "sparsified");
        return SPG_ENOTPD;
    }
    return 0;
}

}  // namespace spg

#include "spg_compat.inc"
#include "spg_propose.inc"
#include "spg_removals.inc"
