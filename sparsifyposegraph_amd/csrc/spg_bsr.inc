// csrc/spg_bsr.inc — the Gauss-Newton information in block-CSR form on the device (included by spg_dense.hip):
// a third sink of dense_assemble_kernel, the product H X (bsr_spmv_kernel) and a block-Jacobi preconditioned
// conjugate-gradient solver as a third LMLinear (g2o's PCG solver family; the reference's own export of the matrix
// is GraphWrapperG2O::sparseInformation, src/graph_wrapper_g2o.cpp:382-396). DESIGN.md 5i.
//
// Layout (spg_bsr_pattern.hpp): D x D row-major blocks, block rows / columns = the variables by ascending pos, both
// triangles stored, columns ascending within a row. Everything is fp64, free of atomics and reduces in a fixed order:
// the same input gives the same bits.
#include "spg_bsr_pattern.hpp"

namespace {

struct BsrDev {
    const int64_t *row_ptr;   // nb + 1
    const int32_t *col;       // nnzb
    const int64_t *diag;      // nb: index of block (i, i)
    double *blocks;           // nnzb * D * D
    int nb;
};

// index of block (i, j), -1 if it is not in the pattern
__device__ __forceinline__ int64_t bsr_find(const BsrDev &B, int i, int j) {
    int64_t lo = B.row_ptr[i], hi = B.row_ptr[i + 1] - 1;
    while (lo <= hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int q = B.col[mid];
        if (q == j) return mid;
        if (q < j) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

// Sink of the assembly kernel that writes block-CSR: like the dense sink it receives the lower block triangle
// (pos(u) < pos(v)) and the diagonal blocks; bsr_mirror_kernel fills the rest.
struct BsrSink {
    BsrDev B;
    int D;
    int *bad;
    __device__ __forceinline__ void add(int pv, int pu, int r, int c, double val) {
        const int64_t k = bsr_find(B, pv / D, pu / D);
        if (k < 0) { *bad = 2; return; }
        B.blocks[k * D * D + r * D + c] += val;
    }
    __device__ __forceinline__ void diag(int pv, int r, int c, double val) { B.blocks[B.diag[pv / D] * D * D + r * D + c] = val; }
    __device__ __forceinline__ void finish(int, int) {}
};

// Upper block triangle <- transpose of the lower one, and the upper triangle of every diagonal block <- its lower one:
// what hip_dense_information does on the host when it mirrors the dense matrix, so block (u, v) is the transpose of
// block (v, u) bit for bit. One wavefront per block row, one lane per entry of a block.
template <int D>
__global__ __launch_bounds__(64) void bsr_mirror_kernel(BsrDev B, int *bad) {
    constexpr int DD = D * D;
    const int i = blockIdx.x, tid = threadIdx.x;
    if (tid >= DD) return;
    const int r = tid / D, c = tid - r * D;
    for (int64_t k = B.row_ptr[i]; k < B.row_ptr[i + 1]; k++) {
        const int j = B.col[k];
        if (j < i) continue;
        if (j == i) {
            if (r < c) B.blocks[k * DD + tid] = B.blocks[k * DD + c * D + r];
            continue;
        }
        const int64_t t = bsr_find(B, j, i);
        if (t < 0) { *bad = 2; continue; }
        B.blocks[k * DD + tid] = B.blocks[t * DD + c * D + r];
    }
}

// Device scalars of one PCG solve. rz and conv are double-buffered by the parity of the iteration: a kernel reads the
// word of its own iteration and only pcg_direction_kernel writes the word of the next one, so no launch reads a word
// that the same launch writes.
struct PcgScal {
    double rz[2];      // r . z
    double bb, rr;     // ||b||^2, ||r||^2 (of the recurrence)
    int conv[2];       // ||r|| <= rel_tol ||b||: the remaining launches return at once
    int iters;         // iterations that changed the iterate
    int breakdown;     // a preconditioner pivot or p^T A p was not positive (also raised in the caller's `bad`)
};

// Y = (H + lambda I) X for the vector blockIdx.y of X. A block row belongs to LPR = 16 (SE2) or 32 (SE3) lanes: S = 5
// slots of D lanes, lane (slot s, row r) multiplies row r of the blocks s, s + S, ... of the block row (rows longer than
// one pass — a hub vertex — are looped over), then slot 0 adds the slots in ascending order. 15 of 16 / 30 of 32 lanes
// work for either D, and the lanes of a pass read 5 consecutive blocks (360 B / 1440 B) of the value array.
template <int D>
__global__ __launch_bounds__(256) void bsr_spmv_kernel(BsrDev B, double lambda, const double *X, double *Y, const PcgScal *sc, int parity) {
    constexpr int DD = D * D, LPR = (D == 3) ? 16 : 32, S = LPR / D, RPW = 256 / LPR;
    if (sc && (sc->conv[parity] || sc->breakdown)) return;
    const int tid = threadIdx.x, sub = tid & (LPR - 1), s = sub / D, r = sub - s * D;
    const int row = blockIdx.x * RPW + tid / LPR;
    const long long n = (long long)D * B.nb;
    const double *x = X + blockIdx.y * n;
    double *y = Y + blockIdx.y * n;
    const bool live = row < B.nb && s < S;
    double acc = 0;
    if (live) {
        const int64_t k1 = B.row_ptr[row + 1];
        for (int64_t k = B.row_ptr[row] + s; k < k1; k += S) {
            const double *blk = B.blocks + k * DD + r * D;
            const double *xv = x + (long long)B.col[k] * D;
#pragma unroll
            for (int c = 0; c < D; c++) acc += blk[c] * xv[c];
        }
    }
    const int base = (tid & 63) & ~(LPR - 1);
    double tot = acc;
#pragma unroll
    for (int t = 1; t < S; t++) tot += __shfl(acc, base + t * D + r, 64);
    if (live && s == 0) {
        if (lambda != 0.0) tot += lambda * x[(long long)row * D + r];
        y[(long long)row * D + r] = tot;
    }
}

// out[slot] = max |diagonal entry| of H (one workgroup, as max_diag_kernel)
template <int D>
__global__ __launch_bounds__(256) void bsr_max_diag_kernel(BsrDev B, double *out, int slot) {
    __shared__ double red[256];
    double s = 0;
    const long long n = (long long)D * B.nb;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const long long q = i / D;
        const int r = (int)(i - q * D);
        s = fmax(s, fabs(B.blocks[B.diag[q] * D * D + r * D + r]));
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[slot] = red[0];
}

// Block-Jacobi preconditioner: Minv_i = (H_ii + lambda I)^-1 by a Cholesky of the D x D block, one lane per block
// (everything in registers). A pivot that is not positive raises *bad, as a failed factorisation does.
template <int D>
__global__ __launch_bounds__(64) void bsr_block_jacobi_kernel(BsrDev B, double lambda, double *Minv, int *bad, PcgScal *sc) {
    constexpr int DD = D * D;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B.nb) return;
    const double *A = B.blocks + B.diag[i] * DD;
    double L[DD], Li[DD];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < D; j++) {
        double d = A[j * D + j] + lambda;
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[j * D + k] * L[j * D + k];
        if (!(d > 0.0) || !isfinite(d)) { ok = false; d = 1.0; }
        const double l = sqrt(d), il = 1.0 / l;
        L[j * D + j] = l;
#pragma unroll
        for (int r = j + 1; r < D; r++) {
            double v = A[r * D + j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[r * D + k] * L[j * D + k];
            L[r * D + j] = v * il;
        }
    }
    // Li = L^-1 (lower), column by column
#pragma unroll
    for (int c = 0; c < D; c++) {
#pragma unroll
        for (int r = 0; r < D; r++) {
            if (r < c) { Li[r * D + c] = 0.0; continue; }
            double v = (r == c) ? 1.0 : 0.0;
#pragma unroll
            for (int k = c; k < r; k++) v -= L[r * D + k] * Li[k * D + c];
            Li[r * D + c] = v / L[r * D + r];
        }
    }
    // Minv = Li^T Li, the lower triangle computed and mirrored
    double *M = Minv + (long long)i * DD;
#pragma unroll
    for (int r = 0; r < D; r++)
#pragma unroll
        for (int c = 0; c <= r; c++) {
            double v = 0;
#pragma unroll
            for (int k = r; k < D; k++) v += Li[k * D + r] * Li[k * D + c];
            M[r * D + c] = v;
            M[c * D + r] = v;
        }
    if (!ok) { *bad = 1; sc->breakdown = 1; }
}

// sum of one value per thread over the workgroup in a fixed order (as sum_kernel); red: 256 doubles of LDS
__device__ __forceinline__ double pcg_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
// sum of the G partial sums a previous launch left, recomputed by every workgroup that needs it (same order, same bits)
__device__ __forceinline__ double pcg_total(const double *partial, int G, double *red) {
    double s = 0;
    for (int i = threadIdx.x; i < G; i += 256) s += partial[i];
    return pcg_block_sum(s, red);
}

// partial[g] = sum of a[i] b[i] over the elements of workgroup g (grid-stride)
__global__ __launch_bounds__(256) void pcg_dot_kernel(const double *a, const double *b, long long n, double *partial, const PcgScal *sc, int parity) {
    __shared__ double red[256];
    if (sc->conv[parity] || sc->breakdown) return;
    double s = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) s += a[i] * b[i];
    s = pcg_block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// alpha = r.z / p.Ap (p.Ap from pcg_dot_kernel's partial sums); x += alpha p, r -= alpha Ap, z = Minv r; partial2[g] and
// partial2[G + g] = this workgroup's share of r.z and r.r. One lane per block of D unknowns (the preconditioner couples
// them). first: x = 0, r = b instead. p.Ap <= 0: nothing is changed, *bad is raised.
template <int D>
__global__ __launch_bounds__(256) void pcg_update_kernel(int nb, const double *Minv, const double *partial, PcgScal *sc, int parity, int first,
                                                         const double *b, double *x, double *r, const double *p, const double *Ap, double *z,
                                                         double *partial2, int *bad) {
    constexpr int DD = D * D;
    __shared__ double red[256];
    const int G = gridDim.x;
    double alpha = 0;
    if (!first) {
        if (sc->conv[parity]) return;
        const double pAp = pcg_total(partial, G, red);
        if (!(pAp > 0.0) || !isfinite(pAp)) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { *bad = 1; sc->breakdown = 1; }
            return;
        }
        alpha = sc->rz[parity] / pAp;
    }
    double rz = 0, rr = 0;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nb; q += (long long)G * 256) {
        double rn[D];
#pragma unroll
        for (int c = 0; c < D; c++) {
            const long long j = q * D + c;
            if (first) { rn[c] = b[j]; x[j] = 0.0; }
            else { rn[c] = r[j] - alpha * Ap[j]; x[j] += alpha * p[j]; }
            r[j] = rn[c];
        }
        const double *M = Minv + q * DD;
#pragma unroll
        for (int a = 0; a < D; a++) {
            double v = 0;
#pragma unroll
            for (int c = 0; c < D; c++) v += M[a * D + c] * rn[c];
            z[q * D + a] = v;
            rz += rn[a] * v;
            rr += rn[a] * rn[a];
        }
    }
    rz = pcg_block_sum(rz, red);
    rr = pcg_block_sum(rr, red);
    if (threadIdx.x == 0) { partial2[blockIdx.x] = rz; partial2[G + blockIdx.x] = rr; }
}

// beta = r.z (new) / r.z (old), p = z + beta p; thread 0 of workgroup 0 keeps the scalars: r.z and the convergence word
// of the next iteration, ||r||^2, the iteration count. first: p = z, ||b||^2 = ||r||^2.
__global__ __launch_bounds__(256) void pcg_direction_kernel(long long n, const double *partial2, PcgScal *sc, int parity, int first, double tol2,
                                                            const double *z, double *p) {
    __shared__ double red[256];
    const int G = gridDim.x;
    const bool keeper = blockIdx.x == 0 && threadIdx.x == 0;
    if (!first && (sc->conv[parity] || sc->breakdown)) {
        if (keeper) sc->conv[parity ^ 1] = sc->conv[parity];
        return;
    }
    const double rz = pcg_total(partial2, G, red), rr = pcg_total(partial2 + G, G, red);
    const double beta = first ? 0.0 : rz / sc->rz[parity];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)G * 256) p[i] = first ? z[i] : z[i] + beta * p[i];
    if (keeper) {
        if (first) sc->bb = rr; else sc->iters++;
        sc->rr = rr;
        sc->rz[parity ^ 1] = rz;
        sc->conv[parity ^ 1] = (rr <= tol2 * sc->bb) ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------ host side
// The pattern on the device and the value array (zeroed by assemble)
struct BsrBufs {
    DevBuf row_ptr, col, diag, blocks, sink_bad;
    BsrDev dev{};
    int D = 0;
    int64_t nnzb = 0;
    int init(int D_, const spg::bsr::Pattern &P, hipStream_t s, char *err, size_t errlen) {
        D = D_; nnzb = P.nnzb();
        int rc;
        if ((rc = upload(row_ptr, P.row_ptr.data(), P.row_ptr.size(), s)) || (rc = upload(col, P.col.data(), P.col.size(), s)) ||
            (rc = upload(diag, P.diag.data(), P.diag.size(), s))) {
            snprintf(err, errlen, "uploading the block-CSR pattern failed (%d)", rc);
            return rc;
        }
        const size_t bytes = (size_t)std::max<int64_t>(nnzb, 1) * D * D * 8;
        if (hipMalloc(&blocks.p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            snprintf(err, errlen, "block-CSR information: %lld blocks (%.1f MB) do not fit in free device memory", (long long)nnzb, 1e-6 * (double)bytes);
            return SPG_ECAPACITY;
        }
        HIPCHK(hipMalloc(&sink_bad.p, sizeof(int)));
        HIPCHK(hipMemsetAsync(sink_bad.p, 0, sizeof(int), s));
        dev = BsrDev{(const int64_t *)row_ptr.p, (const int32_t *)col.p, (const int64_t *)diag.p, (double *)blocks.p, P.nb};
        return 0;
    }
    // blocks <- H of the staged graph (gb.pos = D * block row), optionally b
    int assemble(hipStream_t s, const GraphBufs &gb, double *b) {
        if (hipMemsetAsync(blocks.p, 0, (size_t)std::max<int64_t>(nnzb, 1) * D * D * 8, s) != hipSuccess) return SPG_EHIP;
        if (dev.nb == 0) return 0;
        const BsrSink sink{dev, D, (int *)sink_bad.p};
        by_dim(D, [&](auto d) {
            constexpr int DIM = decltype(d)::value;
            launch_assemble_into<DIM>(gb, sink, s, b);
            hipLaunchKernelGGL((bsr_mirror_kernel<DIM>), dim3(dev.nb), dim3(64), 0, s, dev, (int *)sink_bad.p);
        });
        return 0;
    }
    // Y = (H + lambda I) X, nrhs vectors one after the other (device pointers)
    void apply(hipStream_t s, double lambda, const double *X, double *Y, int nrhs, const PcgScal *sc = nullptr, int parity = 0) const {
        if (dev.nb == 0) return;
        const long long n = (long long)D * dev.nb;
        by_dim(D, [&](auto d) {
            constexpr int DIM = decltype(d)::value, RPW = 256 / ((DIM == 3) ? 16 : 32);
            for (int r0 = 0; r0 < nrhs; r0 += 32768)
                hipLaunchKernelGGL((bsr_spmv_kernel<DIM>), dim3((dev.nb + RPW - 1) / RPW, std::min(32768, nrhs - r0)), dim3(256), 0, s, dev, lambda,
                                   X + r0 * n, Y + r0 * n, sc, parity);
        });
    }
};

// PCG on (H + lambda I) x = b for LM: block-Jacobi preconditioner, the matrix itself is never changed. alpha, beta and
// the norms stay on the device; the host reads the scalars once per kCheck iterations.
struct PcgLM : LMLinear {
    static constexpr int kCheck = 16;
    BsrBufs bsr;
    DevBuf Minv, r, z, p, Ap, partial, partial2, sc;
    int D = 0, nb = 0, G = 1, max_iter = 0;
    long long n = 0;
    double rel_tol = 1e-10;
    spg_pcg_stats *stats = nullptr;
    int init(int D_, const spg::bsr::Pattern &P, double rel_tol_, int max_iter_, spg_pcg_stats *stats_, hipStream_t s, char *err, size_t errlen) {
        D = D_; nb = P.nb; n = (long long)D * nb; rel_tol = rel_tol_; max_iter = max_iter_; stats = stats_;
        G = std::max(1, std::min(256, (nb + 255) / 256));
        if (int rc = bsr.init(D, P, s, err, errlen)) return rc;
        const size_t vec = (size_t)std::max<long long>(n, 1) * 8;
        HIPCHK(hipMalloc(&Minv.p, (size_t)std::max(nb, 1) * D * D * 8));
        HIPCHK(hipMalloc(&r.p, vec));
        HIPCHK(hipMalloc(&z.p, vec));
        HIPCHK(hipMalloc(&p.p, vec));
        HIPCHK(hipMalloc(&Ap.p, vec));
        HIPCHK(hipMalloc(&partial.p, (size_t)G * 8));
        HIPCHK(hipMalloc(&partial2.p, (size_t)2 * G * 8));
        HIPCHK(hipMalloc(&sc.p, sizeof(PcgScal)));
        return 0;
    }
    int build(hipStream_t s, const GraphBufs &gb, double *b, double *scal, char *err, size_t errlen) override {
        if (int rc = bsr.assemble(s, gb, b)) { snprintf(err, errlen, "block-CSR assembly failed"); return rc; }
        by_dim(D, [&](auto d) { hipLaunchKernelGGL((bsr_max_diag_kernel<decltype(d)::value>), dim3(1), dim3(256), 0, s, bsr.dev, scal, 1); });
        return 0;
    }
    int solve(hipStream_t s, const GraphBufs &, double lambda, const double *b, double *sol, int *bad, char *err, size_t errlen) override {
        const auto t0 = std::chrono::steady_clock::now();
        PcgScal *d_sc = (PcgScal *)sc.p;
        const double tol2 = rel_tol * rel_tol;
        HIPCHK(hipMemsetAsync(sc.p, 0, sizeof(PcgScal), s));
        by_dim(D, [&](auto d) {
            constexpr int DIM = decltype(d)::value;
            hipLaunchKernelGGL((bsr_block_jacobi_kernel<DIM>), dim3((nb + 63) / 64), dim3(64), 0, s, bsr.dev, lambda, (double *)Minv.p, bad, d_sc);
            hipLaunchKernelGGL((pcg_update_kernel<DIM>), dim3(G), dim3(256), 0, s, nb, (const double *)Minv.p, (const double *)partial.p, d_sc, 1, 1, b, sol,
                               (double *)r.p, (const double *)p.p, (const double *)Ap.p, (double *)z.p, (double *)partial2.p, bad);
        });
        hipLaunchKernelGGL(pcg_direction_kernel, dim3(G), dim3(256), 0, s, n, (const double *)partial2.p, d_sc, 1, 1, tol2, (const double *)z.p, (double *)p.p);
        PcgScal h{};
        int k = 0;
        bool done = false;
        while (!done) {
            const int stop = std::min(max_iter, k + kCheck);
            for (; k < stop; k++) {
                const int par = k & 1;
                bsr.apply(s, lambda, (const double *)p.p, (double *)Ap.p, 1, d_sc, par);
                hipLaunchKernelGGL(pcg_dot_kernel, dim3(G), dim3(256), 0, s, (const double *)p.p, (const double *)Ap.p, n, (double *)partial.p, d_sc, par);
                by_dim(D, [&](auto d) {
                    hipLaunchKernelGGL((pcg_update_kernel<decltype(d)::value>), dim3(G), dim3(256), 0, s, nb, (const double *)Minv.p, (const double *)partial.p, d_sc,
                                       par, 0, b, sol, (double *)r.p, (const double *)p.p, (const double *)Ap.p, (double *)z.p, (double *)partial2.p, bad);
                });
                hipLaunchKernelGGL(pcg_direction_kernel, dim3(G), dim3(256), 0, s, n, (const double *)partial2.p, d_sc, par, 0, tol2, (const double *)z.p, (double *)p.p);
            }
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&h, sc.p, sizeof(PcgScal), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            done = h.conv[k & 1] || h.breakdown || k >= max_iter;
        }
        if (stats) {
            stats->solves++;
            stats->iterations += h.iters;
            if (!h.conv[k & 1] && !h.breakdown) stats->unconverged++;
            stats->last_rel_residual = h.bb > 0 ? std::sqrt(h.rr / h.bb) : 0.0;
            stats->solve_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        return 0;
    }
};

int bsr_sink_flag(const BsrBufs &bb, hipStream_t s, char *err, size_t errlen) {
    int h_bad = 0;
    HIPCHK(hipMemcpyAsync(&h_bad, bb.sink_bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h_bad) { snprintf(err, errlen, "block-CSR assembly: a block of the information lies outside the pattern"); return SPG_EINVAL; }
    return 0;
}

}  // namespace

namespace spg {

// Values of the block-CSR information over pattern P (built from the same staged graph, in.pos = D * block row): host
// output P.nnzb() * D * D doubles.
int hip_bsr_information(void *stream, const DenseGraphIn &in, const bsr::Pattern &P, double *blocks, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    GraphBufs gb;
    BsrBufs bb;
    if (int rc = bb.init(in.D, P, s, err, errlen)) return rc;
    if (int rc = stage_graph(in, gb, s)) { snprintf(err, errlen, "staging the graph for the block-CSR assembly failed (%d)", rc); return rc; }
    if (int rc = bb.assemble(s, gb, nullptr)) { snprintf(err, errlen, "block-CSR assembly failed"); return rc; }
    HIPCHK(hipGetLastError());
    if (P.nnzb() > 0) HIPCHK(hipMemcpyAsync(blocks, bb.blocks.p, (size_t)P.nnzb() * in.D * in.D * 8, hipMemcpyDeviceToHost, s));
    return bsr_sink_flag(bb, s, err, errlen);
}

// Y = H X for nrhs host vectors of length D * P.nb stored one after the other; H is assembled block-CSR and never leaves the device
int hip_bsr_apply(void *stream, const DenseGraphIn &in, const bsr::Pattern &P, const double *X, int nrhs, double *Y, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    const size_t len = (size_t)in.D * P.nb * (size_t)nrhs;
    if (len == 0) return 0;
    GraphBufs gb;
    BsrBufs bb;
    DevBuf dx, dy;
    if (int rc = bb.init(in.D, P, s, err, errlen)) return rc;
    if (int rc = stage_graph(in, gb, s)) { snprintf(err, errlen, "staging the graph for the block-CSR assembly failed (%d)", rc); return rc; }
    if (hipMalloc(&dx.p, len * 8) != hipSuccess || hipMalloc(&dy.p, len * 8) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(err, errlen, "information apply: %d vectors of %d unknowns do not fit in free device memory", nrhs, in.D * P.nb);
        return SPG_ECAPACITY;
    }
    HIPCHK(hipMemcpyAsync(dx.p, X, len * 8, hipMemcpyHostToDevice, s));
    if (int rc = bb.assemble(s, gb, nullptr)) { snprintf(err, errlen, "block-CSR assembly failed"); return rc; }
    bb.apply(s, 0.0, (const double *)dx.p, (double *)dy.p, nrhs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(Y, dy.p, len * 8, hipMemcpyDeviceToHost, s));
    return bsr_sink_flag(bb, s, err, errlen);
}

// optimize() with the PCG solver. in.pos = D * block row for every free vertex, P the pattern of that numbering.
int hip_pcg_optimize(void *stream, const DenseGraphIn &in, const bsr::Pattern &P, int n, int iterations, double rel_tol, int max_iter,
                     spg_optimize_stats &out, spg_pcg_stats &pcg, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    if (n != in.D * P.nb) { snprintf(err, errlen, "hip_pcg_optimize: %d block rows, n = %d", P.nb, n); return SPG_EINVAL; }
    auto lin = std::make_unique<PcgLM>();
    if (int rc = lin->init(in.D, P, rel_tol, max_iter, &pcg, s, err, errlen)) return rc;
    GraphBufs gb;
    if (int rc = stage_graph(in, gb, s)) { snprintf(err, errlen, "staging the graph for the optimiser failed (%d)", rc); return rc; }
    return lm_run(s, in, gb, n, std::max(n, 1), iterations, *lin, out, err, errlen);
}

// (tools/bsr_bench.py) HIP-event times at the staged graph, each the mean of `reps` runs after a warm-up:
// out[0] block-CSR assembly (memset + Jacobians + assembly + mirror), out[1] one product H x, out[2] the assembly of
// the same graph into the fronts of the sparse solver's plan, all in ms; out[3] = blocks.
int hip_bsr_bench(void *stream, const DenseGraphIn &in, const bsr::Pattern &P, int reps, double *out, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    const int D = in.D, nb = P.nb;
    if (nb == 0 || reps <= 0) return SPG_EINVAL;
    GraphBufs gb;
    BsrBufs bb;
    DevBuf dx, dy;
    if (int rc = bb.init(D, P, s, err, errlen)) return rc;
    if (int rc = stage_graph(in, gb, s)) { snprintf(err, errlen, "staging the graph failed (%d)", rc); return rc; }
    const size_t vec = (size_t)D * nb * 8;
    HIPCHK(hipMalloc(&dx.p, vec));
    HIPCHK(hipMalloc(&dy.p, vec));
    {
        std::vector<double> ones((size_t)D * nb, 1.0);
        HIPCHK(hipMemcpy(dx.p, ones.data(), vec, hipMemcpyHostToDevice));
    }
    EventTimer timer;
    auto timed = [&](auto &&work, double &ms_out) -> int {
        work();   // warm-up
        HIPCHK(timer.start(s));
        for (int i = 0; i < reps; i++) work();
        HIPCHK(timer.stop(s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        float ms = 0;
        HIPCHK(timer.ms(ms));
        ms_out = (double)ms / reps;
        return 0;
    };
    if (int rc = timed([&] { (void)bb.assemble(s, gb, nullptr); }, out[0])) return rc;
    if (int rc = timed([&] { bb.apply(s, 0.0, (const double *)dx.p, (double *)dy.p, 1); }, out[1])) return rc;
    // the fronts of the graph's own plan, set up as hip_sparse_optimize does
    std::vector<int32_t> block_of((size_t)in.nv, -1), pos_new((size_t)in.nv, -1);
    for (int v = 0; v < in.nv; v++) if (in.pos[v] >= 0) block_of[v] = in.pos[v] / D;
    sparse::BlockGraph bg;
    block_graph_of(in, block_of, nb, bg);
    sparse::Plan plan;
    sparse::build_plan(bg, D, nullptr, sparse_leaf(D), plan);
    for (int v = 0; v < in.nv; v++) if (block_of[v] >= 0) pos_new[v] = D * plan.iperm[block_of[v]];
    DenseGraphIn in2 = in;
    in2.pos = pos_new.data();
    auto sp = std::make_unique<SparseSolver>();
    if (int rc = sp->init(std::move(plan), false, err, errlen)) return rc;
    GraphBufs gb2;
    if (int rc = stage_graph(in2, gb2, s)) { snprintf(err, errlen, "staging the graph failed (%d)", rc); return rc; }
    if (int rc = timed([&] { (void)sp->assemble(s, gb2, nullptr, nullptr); }, out[2])) return rc;
    out[3] = (double)P.nnzb();
    return 0;
}

}  // namespace spg
