// csrc/spg_compat.inc — joint compatibility of loop-closure candidates (spg_graph_compatible_candidates, spg_ctx_max_clique;
// DESIGN 5g-C). Included at the end of spg_sparse.inc: the rel_* steps, sel_load_sigma, cov_solve_device and the host
// helpers are those of the selection. Nothing of the selection is edited: its kernels and SelArgs keep their text.
//
// Per candidate i (a hypothetical binary edge with Omega_i = L_i L_i^T, J_i = [Ja Jb], e_i at the stored estimates):
// U_i = L_i^T J_i (D x 2D), w_i = L_i^T e_i, M_ij = delta_ij I + U_i Sigma_(ai bi),(aj bj) U_j^T. For a set S,
// d2(S) = w_S^T M_SS^-1 w_S; M_SS >= I. Three stages on the device, no host round trip between them:
//   1. sp_compat_init_kernel (U, w, M_ii and its factor, d2_i, the state) and sp_compat_pair_kernel: d2_ij of every
//      unordered eligible pair by block elimination (i first), both adjacency bits from the one comparison;
//   2. sp_clique_seed_kernel / sp_clique_write_kernel: the greedy largest consistent set over every seed;
//   3. sp_compat_verify_kernel: the sequential joint gate over the clique in ascending d2_i (left-looking block Cholesky).

namespace {

constexpr int kCompatMaxN = 16384;   // candidates / vertices of a consistency graph: 256 adjacency words per row
constexpr int kCompatTileI = 16;     // rows of a pair tile (a divisor of 64: the tile's transposed bits share one word)
constexpr int kVerifyLdsRow = 6144;  // doubles of LDS the verify kernel has for the D rows of a block row

struct CompatArgs {
    const double *arena;
    const int64_t *vpo;
    const int32_t *va, *vb, *sa, *sb;
    const double *rec;        // n x (PS + D (D + 1) / 2)
    const double *joint;      // m D x m D, row stride ld
    long long ld;
    double *U;                // n x D x 2D: L^T [Ja Jb]
    double *w, *z;            // n x D each: L^T e and M_ii^-1 L^T e
    double *M, *G;            // n x D^2 each: M_ii and its Cholesky factor (lower triangle)
    double *d2;               // n
    int32_t *state;           // n: the SPG_CAND_* value the candidate reports
    unsigned long long *adj;  // n x nw, bit j of row i
    int nw;
    double *pair_d2;          // n x n, or nullptr
    int n;
    double max_d2, pair_max_d2;
};

// One wavefront per candidate, four per workgroup, the per-wave LDS slice of sp_select_init_kernel: U, w, M_ii = I + U S U^T
// = G G^T, d2_i = |G^-1 w|^2, z = G^-T G^-1 w and the state (Omega not PD: 1; max_d2 > 0 and d2 > max_d2: 2; else 0).
template <int D>
__global__ __launch_bounds__(256) void sp_compat_init_kernel(CompatArgs a) {
    constexpr int W = 2 * D, DD = D * D, PS = (D == 6) ? 7 : 3, TRI = D * (D + 1) / 2, REC = PS + TRI;
    constexpr int PER = W * W + 2 * DD + 2 * D * W + 2 * DD + 4 * D;
    __shared__ double lds[4 * PER];
    __shared__ int okv[4];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, i = blockIdx.x * 4 + wv;
    const bool act = i < a.n;
    double *S = lds + wv * PER, *Ja = S + W * W, *Jb = Ja + DD, *U = Jb + DD, *T = U + D * W, *L = T + D * W, *M = L + DD, *e = M + DD, *y = e + D,
           *w0 = y + D, *zz = w0 + D;
    const double *rec = act ? a.rec + (long long)i * REC : nullptr;
    if (act) {
        sel_load_sigma<D>(lane, a.joint, a.ld, a.sa[i], a.sb[i], a.sa[i], a.sb[i], S);
        if (lane == 0) rel_geometry<D>(a.arena, a.vpo, a.va[i], a.vb[i], rec, nullptr, Ja, Jb, e);
    }
    __syncthreads();
    if (act && lane == 0) {
        double chi;
        okv[wv] = rel_omega<D>(rec + PS, e, L, y, chi);
    }
    __syncthreads();
    const bool go = act && okv[wv];
    if (go)
        for (int k = lane; k < D * W; k += 64) {   // U = L^T [Ja Jb], L lower triangular
            const int r = k / W, c = k - r * W;
            const double *J = c < D ? Ja : Jb;
            const int cc = c < D ? c : c - D;
            double s = 0;
            for (int t = r; t < D; t++) s += L[t * D + r] * J[t * D + cc];
            U[k] = s;
        }
    __syncthreads();
    if (go)
        for (int k = lane; k < D * W; k += 64) {   // T = U S
            const int r = k / W, c = k - r * W;
            double s = 0;
            for (int t = 0; t < W; t++) s += U[r * W + t] * S[t * W + c];
            T[k] = s;
        }
    __syncthreads();
    if (go && lane < DD) {                          // M = I + T U^T, r <= c, mirrored
        const int r = lane / D, c = lane - r * D;
        if (r <= c) {
            double s = (r == c) ? 1.0 : 0.0;
            for (int t = 0; t < W; t++) s += T[r * W + t] * U[c * W + t];
            M[r * D + c] = s;
            M[c * D + r] = s;
        }
    }
    __syncthreads();
    if (go && lane < DD) a.M[(long long)i * DD + lane] = M[lane];
    if (go && lane < D) w0[lane] = y[lane];
    __syncthreads();
    if (act && lane == 0) {
        double gain, d2 = __builtin_nan("");
        int st = 1;
        if (go) {
            rel_chol_M<D>(M, y, gain, d2);          // y <- G^-1 w
            for (int j = D - 1; j >= 0; j--) {       // zz = G^-T y
                double v = y[j];
                for (int k = j + 1; k < D; k++) v -= M[k * D + j] * zz[k];
                zz[j] = v / M[j * D + j];
            }
            st = (a.max_d2 > 0.0 && !(d2 <= a.max_d2)) ? 2 : 0;
        }
        a.d2[i] = d2;
        a.state[i] = st;
    }
    __syncthreads();
    if (go) {
        for (int k = lane; k < D * W; k += 64) a.U[(long long)i * D * W + k] = U[k];
        if (lane < DD) a.G[(long long)i * DD + lane] = M[lane];   // the lower triangle is the factor
        if (lane < D) {
            a.w[(long long)i * D + lane] = w0[lane];
            a.z[(long long)i * D + lane] = zz[lane];
        }
    }
}

// Stage 1. One workgroup per tile of 16 candidates i by 64 candidates j, tiles that reach above the diagonal only; U, G and
// z of the 16 rows and U of the 64 columns are staged in LDS (column rows padded by one double). Wavefront w takes rows
// 4w .. 4w + 3 one after the other, lane l the column j0 + l: one pair per lane, the D x D blocks in registers. For i < j,
// both eligible:
//   M_ij = U_i Sigma_(ai bi),(aj bj) U_j^T                     the four Sigma blocks row by row from the joint block
//   X = G_ii^-1 M_ij,  v = w_j - M_ij^T z_i,  G G^T = M_jj - X^T X,  d2_ij = d2_i + |G^-1 v|^2
// (a factorisation that breaks down gives NaN: inconsistent). The lane's column is bit l of word j0 / 64 of row i, so the
// wavefront's ballot is that word's contribution; the transposed bits (row j, the 16 columns i0 .. i0 + 15 of one word) are
// gathered from the 16 ballots by the first wavefront. Both go out by one 64-bit atomicOr per word: a row's word also
// receives bits from other tiles. One predicate sets bit (i, j) and bit (j, i).
template <int D>
__global__ __launch_bounds__(256) void sp_compat_pair_kernel(CompatArgs a) {
    constexpr int W = 2 * D, DD = D * D, DW = D * W, TI = kCompatTileI;
    __shared__ double Uj[64 * (DW + 1)];
    __shared__ double Ui[TI * DW], Gi[TI * DD], zi[TI * D];
    __shared__ unsigned long long sbal[TI];
    const int i0 = blockIdx.y * TI, j0 = blockIdx.x * 64;
    if (j0 + 63 <= i0) return;   // no pair i < j in this tile (uniform over the workgroup)
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    for (int k = tid; k < 64 * DW; k += 256) {
        const int jj = k / DW, q = k - jj * DW;
        Uj[jj * (DW + 1) + q] = (j0 + jj < a.n && a.state[j0 + jj] == 0) ? a.U[(long long)(j0 + jj) * DW + q] : 0.0;
    }
    for (int k = tid; k < TI * DW; k += 256) {
        const int ii = k / DW;
        const bool ok = i0 + ii < a.n && a.state[i0 + ii] == 0;
        Ui[k] = ok ? a.U[(long long)i0 * DW + k] : 0.0;
        if (k < TI * DD) Gi[k] = (i0 + k / DD < a.n && a.state[i0 + k / DD] == 0) ? a.G[(long long)i0 * DD + k] : 1.0;
        if (k < TI * D) zi[k] = (i0 + k / D < a.n && a.state[i0 + k / D] == 0) ? a.z[(long long)i0 * D + k] : 0.0;
    }
    __syncthreads();
    const int j = j0 + lane;
    const bool jok = j < a.n && a.state[j] == 0;
    const int saj = jok ? a.sa[j] : -1, sbj = jok ? a.sb[j] : -1;
    const double *uj = Uj + lane * (DW + 1);
#pragma unroll 1
    for (int rr = 0; rr < 4; rr++) {
        const int ii = wv * 4 + rr, i = i0 + ii;
        const bool iok = i < a.n && a.state[i] == 0;   // uniform over the wavefront
        const bool pair = iok && jok && j > i;
        bool consistent = false;
        if (pair) {
            const int sai = a.sa[i], sbi = a.sb[i];
            const double *ui = Ui + ii * DW, *gi = Gi + ii * DD;
            double Mij[D][D];
#pragma unroll
            for (int r = 0; r < D; r++)
#pragma unroll
                for (int c = 0; c < D; c++) Mij[r][c] = 0.0;
#pragma unroll
            for (int p = 0; p < W; p++) {
                const int br = p < D ? sai : sbi, pr = p < D ? p : p - D;
                if (br < 0) continue;
                const double *row = a.joint + ((long long)br * D + pr) * a.ld;
                double y[D];
#pragma unroll
                for (int c = 0; c < D; c++) y[c] = 0.0;
#pragma unroll
                for (int q = 0; q < W; q++) {
                    const int bc = q < D ? saj : sbj, qc = q < D ? q : q - D;
                    const double sv = bc < 0 ? 0.0 : row[(long long)bc * D + qc];
#pragma unroll
                    for (int c = 0; c < D; c++) y[c] += sv * uj[c * W + q];
                }
#pragma unroll
                for (int r = 0; r < D; r++)
#pragma unroll
                    for (int c = 0; c < D; c++) Mij[r][c] += ui[r * W + p] * y[c];
            }
            double v[D];
#pragma unroll
            for (int c = 0; c < D; c++) {
                double s = a.w[(long long)j * D + c];
#pragma unroll
                for (int r = 0; r < D; r++) s -= Mij[r][c] * zi[ii * D + r];
                v[c] = s;
            }
#pragma unroll
            for (int c = 0; c < D; c++)              // X = G_ii^-1 M_ij, in place
#pragma unroll
                for (int r = 0; r < D; r++) {
                    double x = Mij[r][c];
#pragma unroll
                    for (int k = 0; k < r; k++) x -= gi[r * D + k] * Mij[k][c];
                    Mij[r][c] = x / gi[r * D + r];
                }
            double Sc[D][D];
            const double *mj = a.M + (long long)j * DD;
#pragma unroll
            for (int r = 0; r < D; r++)
#pragma unroll
                for (int c = 0; c <= r; c++) {
                    double s = mj[r * D + c];
#pragma unroll
                    for (int k = 0; k < D; k++) s -= Mij[k][r] * Mij[k][c];
                    Sc[r][c] = s;
                }
            bool ok = true;
            double extra = 0.0;
#pragma unroll
            for (int jc = 0; jc < D; jc++) {        // G G^T = Sc with the forward solve G x = v interleaved
                double d = Sc[jc][jc];
#pragma unroll
                for (int k = 0; k < jc; k++) d -= Sc[jc][k] * Sc[jc][k];
                ok = ok && d > 0.0 && isfinite(d);
                d = sqrt(d);
                Sc[jc][jc] = d;
#pragma unroll
                for (int r = jc + 1; r < D; r++) {
                    double t = Sc[r][jc];
#pragma unroll
                    for (int k = 0; k < jc; k++) t -= Sc[r][k] * Sc[jc][k];
                    Sc[r][jc] = t / d;
                }
                double x = v[jc];
#pragma unroll
                for (int k = 0; k < jc; k++) x -= Sc[jc][k] * v[k];
                x /= d;
                v[jc] = x;
                extra += x * x;
            }
            const double d2ij = ok ? a.d2[i] + extra : __builtin_nan("");
            consistent = d2ij <= a.pair_max_d2;      // NaN: inconsistent
            if (a.pair_d2) {
                a.pair_d2[(long long)i * a.n + j] = d2ij;
                a.pair_d2[(long long)j * a.n + i] = d2ij;
            }
        }
        if (a.pair_d2 && iok && j == i) a.pair_d2[(long long)i * a.n + i] = a.d2[i];
        const unsigned long long bal = __ballot(consistent);
        if (lane == 0) {
            sbal[ii] = bal;
            if (bal) atomicOr(&a.adj[(long long)i * a.nw + blockIdx.x], bal);
        }
    }
    __syncthreads();
    if (tid < 64 && j < a.n) {
        unsigned long long bits = 0;
        for (int ii = 0; ii < TI; ii++) bits |= ((sbal[ii] >> tid) & 1ull) << ((i0 + ii) & 63);
        if (bits) atomicOr(&a.adj[(long long)j * a.nw + (i0 >> 6)], bits);
    }
}

// Stage 2 on any symmetric bit matrix with a clear diagonal: for seed s, R = (s), P = N(s); while P is not empty take
// v = argmax over u in P of |N(u) & P| (ties: the lowest index), append it and set P &= N(v). One wavefront per seed, P in
// LDS; the vertices of P are spread over the lanes, each lane popcounts its row against P (nw independent loads in flight
// per lane), and the argmax is a wavefront reduction on the key (count + 1, ~index). A form with a row's words across a
// group of lanes, read as one contiguous piece and summed by shuffles, was measured three times slower (DESIGN 7): the
// dependent shuffles per vertex cost more than the scattered loads. Returns |R|; WRITE: the members go to out in the order
// they were added.
template <bool WRITE>
__device__ __forceinline__ int clique_grow(const unsigned long long *adj, int n, int nw, int s, unsigned long long *P, int32_t *out, int lane) {
    for (int w = lane; w < nw; w += 64) P[w] = adj[(long long)s * nw + w];
    if (WRITE && lane == 0) out[0] = s;
    int size = 1;
    __syncthreads();
    while (true) {
        int bc = -1, bu = 0;
        for (int u = lane; u < n; u += 64) {
            if (!((P[u >> 6] >> (u & 63)) & 1ull)) continue;
            const unsigned long long *row = adj + (long long)u * nw;
            int c = 0;
            for (int w = 0; w < nw; w++) c += __popcll(row[w] & P[w]);
            if (c > bc) { bc = c; bu = u; }   // u ascends within a lane: the first maximum is the lowest index
        }
        unsigned long long key = bc < 0 ? 0ull : ((unsigned long long)(bc + 1) << 32) | (unsigned long long)(0xffffffffu - (unsigned)bu);
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(key, o, 64);
            key = other > key ? other : key;
        }
        if (key == 0) break;                  // P is empty (the same on every lane)
        const int v = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
        if (WRITE && lane == 0 && size < n) out[size] = v;
        size++;
        __syncthreads();
        for (int w = lane; w < nw; w += 64) P[w] &= adj[(long long)v * nw + w];
        __syncthreads();
    }
    return size;
}

struct CliqueArgs {
    const unsigned long long *adj;
    int n, nw;
    const int32_t *state;        // per vertex, nullptr: every vertex is a seed; else the seeds are those with state 0
    int32_t *degree;             // n, may be nullptr
    unsigned long long *best;    // (size << 32) | ~seed: the largest size, ties to the lowest seed
    int32_t *out;                // n: the members of the winning seed, in order
    int32_t *res;                // [0] size, [1] seed (-1: no seed)
};
// One wavefront per seed. A seed with deg(s) + 1 < the best size found so far is skipped: its set cannot reach that size,
// and under (longest, ties to the lowest seed) a strictly shorter set never wins, so the pruning cannot change the answer,
// whatever order the seeds finish in. The best (size, seed) is one 64-bit atomicMax on the packed key.
__global__ __launch_bounds__(64) void sp_clique_seed_kernel(CliqueArgs a) {
    __shared__ unsigned long long P[kCompatMaxN / 64];
    const int s = blockIdx.x, lane = threadIdx.x;
    int deg = 0;
    for (int w = lane; w < a.nw; w += 64) deg += __popcll(a.adj[(long long)s * a.nw + w]);
    for (int o = 32; o > 0; o >>= 1) deg += __shfl_xor(deg, o, 64);
    if (a.degree && lane == 0) a.degree[s] = deg;
    if (a.state && a.state[s] != 0) return;
    const unsigned long long seen = __hip_atomic_load(a.best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((long long)(seen >> 32) > (long long)deg + 1) return;
    const int size = clique_grow<false>(a.adj, a.n, a.nw, s, P, nullptr, lane);
    if (lane == 0) atomicMax(a.best, ((unsigned long long)size << 32) | (unsigned long long)(0xffffffffu - (unsigned)s));
}
// One wavefront: re-runs the winning seed and writes its members, so that no list is ever written by competing seeds.
__global__ __launch_bounds__(64) void sp_clique_write_kernel(CliqueArgs a) {
    __shared__ unsigned long long P[kCompatMaxN / 64];
    const int lane = threadIdx.x;
    const unsigned long long key = *a.best;
    if (key == 0) {
        if (lane == 0) { a.res[0] = 0; a.res[1] = -1; }
        return;
    }
    const int s = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
    const int size = clique_grow<true>(a.adj, a.n, a.nw, s, P, a.out, lane);
    if (lane == 0) { a.res[0] = size; a.res[1] = s; }
}

struct VerifyArgs {
    const double *U, *w, *M, *d2;
    const int32_t *sa, *sb;
    const double *joint;
    long long ld;
    const int32_t *clique;    // the members, res[0] of them
    const int32_t *res;
    int32_t *order;           // n: the members in ascending (d2, index)
    int32_t *state;
    double *F;                // (kk D)^2, row stride kk D: the transpose of the factor, F[c][t] = G[t][c] for t >= c
    double *rows;             // D x kk D: the block row being formed, when it does not fit in LDS
    double *y;                // kk D: G_SS^-1 w_S
    const double *jmax;       // kk thresholds, or nullptr
    int32_t *acc;             // kk: the accepted candidates in order
    double *jd2;              // kk: d2(S) after each acceptance
    int32_t *nacc;
    int kk;
};
// Stage 3, one workgroup. The members are ranked by (d2_i, index). For member i with p accepted before it:
//   row = M_iS (D x pD, each entry a 2D x 2D contraction read from the joint block), then row <- row G_SS^-T by forward
//   substitution, one wavefront per row r: column c belongs to lane c mod 64, which divides by the diagonal and broadcasts;
//   every lane then updates the later columns it owns from row c of F (contiguous), so no lane reads what another wrote;
//   v = w_i - row y_S, G_ii G_ii^T = M_ii - row row^T, y_i = G_ii^-1 v, t = D2 + |y_i|^2.
// Accepted (no thresholds, or t <= jmax[p]; a factorisation that breaks down or a non-finite t is a rejection): the block
// row becomes columns p D .. of F, y_i is appended, D2 = t. Rejected: the row is simply overwritten by the next member.
template <int D>
__global__ __launch_bounds__(256) void sp_compat_verify_kernel(VerifyArgs a) {
    constexpr int W = 2 * D, DD = D * D, DW = D * W;
    __shared__ double lrow[kVerifyLdsRow];
    __shared__ double Ui[DW], Sc[DD], vv[D], wi[D];
    __shared__ int sp, sdec;
    __shared__ double sD2;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int c = a.res[0], kkD = a.kk * D;
    for (int t = tid; t < c; t += 256) {
        const int i = a.clique[t];
        const double di = a.d2[i];
        int rank = 0;
        for (int u = 0; u < c; u++) {
            const int j = a.clique[u];
            const double dj = a.d2[j];
            rank += (dj < di || (dj == di && j < i)) ? 1 : 0;
        }
        a.order[rank] = i;
    }
    if (tid == 0) { sp = 0; sD2 = 0.0; sdec = 0; }
    __syncthreads();
    double *rowbase = ((long long)D * kkD <= kVerifyLdsRow) ? lrow : a.rows;
    for (int t = 0; t < c; t++) {
        const int p = sp;
        if (p >= a.kk) break;
        const int i = a.order[t], pD = p * D;
        for (int k = tid; k < DW; k += 256) Ui[k] = a.U[(long long)i * DW + k];
        if (tid < D) wi[tid] = a.w[(long long)i * D + tid];
        __syncthreads();
        const int sai = a.sa[i], sbi = a.sb[i];
        for (int el = tid; el < D * pD; el += 256) {       // M_iS
            const int r = el / pD, col = el - r * pD, s = col / D, cc = col - s * D, j = a.acc[s];
            const int saj = a.sa[j], sbj = a.sb[j];
            const double *uj = a.U + (long long)j * DW + cc * W;
            double m = 0.0;
            for (int pp = 0; pp < W; pp++) {
                const int br = pp < D ? sai : sbi, pr = pp < D ? pp : pp - D;
                if (br < 0) continue;
                const double *row = a.joint + ((long long)br * D + pr) * a.ld;
                double yv = 0.0;
                for (int q = 0; q < W; q++) {
                    const int bc = q < D ? saj : sbj, qc = q < D ? q : q - D;
                    if (bc >= 0) yv += row[(long long)bc * D + qc] * uj[q];
                }
                m += Ui[r * W + pp] * yv;
            }
            rowbase[(long long)r * kkD + col] = m;
        }
        __syncthreads();
        for (int r = wv; r < D; r += 4) {                  // row <- row G_SS^-T, then v_r
            double *row = rowbase + (long long)r * kkD;
            for (int col = 0; col < pD; col++) {
                const int owner = col & 63;
                const double *f = a.F + (long long)col * kkD;
                double x = 0.0;
                if (lane == owner) {
                    x = row[col] / f[col];
                    row[col] = x;
                }
                x = __shfl(x, owner, 64);
                for (int u = col + 1 + ((lane - col - 1) & 63); u < pD; u += 64) row[u] -= x * f[u];
            }
            double part = 0.0;
            for (int u = lane; u < pD; u += 64) part += row[u] * a.y[u];
            for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
            if (lane == 0) vv[r] = wi[r] - part;
        }
        __syncthreads();
        for (int e = wv; e < DD; e += 4) {                 // M_ii - row row^T, lower triangle
            const int r = e / D, cc = e - r * D;
            if (cc > r) continue;
            const double *ra = rowbase + (long long)r * kkD, *rb = rowbase + (long long)cc * kkD;
            double part = 0.0;
            for (int u = lane; u < pD; u += 64) part += ra[u] * rb[u];
            for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
            if (lane == 0) Sc[e] = a.M[(long long)i * DD + e] - part;
        }
        __syncthreads();
        if (tid == 0) {
            bool ok = true;
            double extra = 0.0;
            for (int jc = 0; jc < D; jc++) {
                double d = Sc[jc * D + jc];
                for (int k = 0; k < jc; k++) d -= Sc[jc * D + k] * Sc[jc * D + k];
                ok = ok && d > 0.0 && isfinite(d);
                d = sqrt(d);
                Sc[jc * D + jc] = d;
                for (int r = jc + 1; r < D; r++) {
                    double v = Sc[r * D + jc];
                    for (int k = 0; k < jc; k++) v -= Sc[r * D + k] * Sc[jc * D + k];
                    Sc[r * D + jc] = v / d;
                }
                double x = vv[jc];
                for (int k = 0; k < jc; k++) x -= Sc[jc * D + k] * vv[k];
                x /= d;
                vv[jc] = x;
                extra += x * x;
            }
            const double tt = sD2 + extra;
            const bool accept = ok && isfinite(tt) && (!a.jmax || tt <= a.jmax[p]);
            if (accept) {
                a.acc[p] = i;
                a.jd2[p] = tt;
                sD2 = tt;
                for (int r = 0; r < D; r++) a.y[pD + r] = vv[r];
            }
            a.state[i] = accept ? 3 : 4;
            sdec = accept ? 1 : 0;
        }
        __syncthreads();
        if (sdec) {
            for (int el = tid; el < D * pD; el += 256) {
                const int r = el / pD, col = el - r * pD;
                a.F[(long long)col * kkD + pD + r] = rowbase[(long long)r * kkD + col];
            }
            if (tid < DD) {
                const int r = tid / D, cc = tid - r * D;
                if (r >= cc) a.F[(long long)(pD + cc) * kkD + pD + r] = Sc[r * D + cc];
            }
        }
        __syncthreads();
        if (tid == 0 && sdec) sp = p + 1;
        __syncthreads();
    }
    if (tid == 0) *a.nacc = sp;
}

}  // namespace

namespace spg {

// Stage 2 on device buffers: dbest, dout (n) and dres (2) are the caller's; dbest is cleared here.
static void launch_clique(hipStream_t s, const unsigned long long *adj, int n, int nw, const int32_t *state, int32_t *degree, unsigned long long *dbest,
                          int32_t *dout, int32_t *dres) {
    (void)hipMemsetAsync(dbest, 0, sizeof(unsigned long long), s);
    const CliqueArgs ca{adj, n, nw, state, degree, dbest, dout, dres};
    hipLaunchKernelGGL(sp_clique_seed_kernel, dim3((unsigned)n), dim3(64), 0, s, ca);
    hipLaunchKernelGGL(sp_clique_write_kernel, dim3(1), dim3(64), 0, s, ca);
}

// spg_ctx_max_clique: adj (host) is n x ceil(n / 64) words, already checked (symmetric, clear diagonal, no bits at or
// beyond n), 1 <= n <= 16 384. clique: n entries (host), the members in order, -1 beyond *size.
int hip_max_clique(void *stream, int n, const uint64_t *adj, int32_t *clique, int *size, int32_t *seed, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    const int nw = (n + 63) / 64;
    DevBuf dadj, dbest, dout, dres;
    if (int rc = upload(dadj, adj, (size_t)n * nw, s)) {
        snprintf(err, errlen, "staging the consistency graph failed (%d)", rc);
        return rc;
    }
    HIPCHK(hipMalloc(&dbest.p, sizeof(unsigned long long)));
    HIPCHK(hipMalloc(&dout.p, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dres.p, 2 * sizeof(int32_t)));
    HIPCHK(hipMemsetAsync(dout.p, 0xff, (size_t)n * sizeof(int32_t), s));
    launch_clique(s, (const unsigned long long *)dadj.p, n, nw, nullptr, nullptr, (unsigned long long *)dbest.p, (int32_t *)dout.p, (int32_t *)dres.p);
    HIPCHK(hipGetLastError());
    int32_t res[2] = {0, -1};
    HIPCHK(hipMemcpyAsync(res, dres.p, sizeof res, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(clique, dout.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *size = res[0];
    *seed = res[1];
    return 0;
}

// spg_graph_compatible_candidates: the sub-block lists, the poses ca / cb and the slots sa / sb as hip_sparse_select (the
// joint block alone). The tail enqueues init, the pair tiles, the clique kernels and the verify kernel without a
// synchronisation. Host arrays: out.compatible / joint_d2: kk entries (-1 / NaN beyond *ncompat); clique, d2, degree,
// status: n each, pair_d2: n x n, each may be nullptr.
int hip_sparse_compat(void *stream, const DenseGraphIn &in, const int32_t *va, const int32_t *vb, const int64_t *dst, int32_t ld, int64_t nblk,
                      int64_t joint_len, const int32_t *ca, const int32_t *cb, const int32_t *sa, const int32_t *sb, int n, const double *rec, int kk,
                      double max_d2, double pair_max_d2, const double *joint_max_d2, const CompatOut &out, int *ncompat, spg_compat_stats &stats,
                      char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    const int D = in.D, DD = D * D, DW = 2 * DD, PS = D == 6 ? 7 : 3, REC = PS + D * (D + 1) / 2;
    const int nw = (n + 63) / 64;
    const int64_t kkD = (int64_t)kk * D;
    int rc = 0;
    {   // free HBM, before anything is allocated
        const double b_joint = 8.0 * (double)joint_len, b_cand = 8.0 * (double)n * (DW + 2 * D + 2 * DD + 4), b_adj = 8.0 * (double)n * nw,
                     b_fact = 8.0 * ((double)kkD * kkD + (double)(D + 1) * kkD), b_pair = out.pair_d2 ? 8.0 * (double)n * n : 0.0;
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        if (b_joint + b_cand + b_adj + b_fact + b_pair + (double)(1ull << 30) > (double)free_b) {
            snprintf(err, errlen,
                     "candidate compatibility needs %.2f GB for the joint covariance of the endpoints, %.2f GB for the consistency graph, %.2f GB for the "
                     "joint factor of min(k, n) = %d candidates and %.2f GB for pair_d2, %.1f GB are free",
                     b_joint * 1e-9, b_adj * 1e-9, b_fact * 1e-9, kk, b_pair * 1e-9, free_b * 1e-9);
            return SPG_ECAPACITY;
        }
    }
    DevBuf djoint, dca, dcb, dsa, dsb, drec, dU, dw, dz, dM, dG, dd2, dstate, dadj, dpair, ddeg, dbest, dclq, dres, dorder, dF, drows, dy, djmax, dacc, djd2,
        dnacc;
    if ((rc = upload(dca, ca, (size_t)n, s)) || (rc = upload(dcb, cb, (size_t)n, s)) || (rc = upload(dsa, sa, (size_t)n, s)) ||
        (rc = upload(dsb, sb, (size_t)n, s)) || (rc = upload(drec, rec, (size_t)n * REC, s)) ||
        (joint_max_d2 && (rc = upload(djmax, joint_max_d2, (size_t)kk, s)))) {
        snprintf(err, errlen, "staging the candidates failed (%d)", rc);
        return rc;
    }
    HIPCHK(hipMalloc(&dU.p, (size_t)n * DW * 8));
    HIPCHK(hipMalloc(&dw.p, (size_t)n * D * 8));
    HIPCHK(hipMalloc(&dz.p, (size_t)n * D * 8));
    HIPCHK(hipMalloc(&dM.p, (size_t)n * DD * 8));
    HIPCHK(hipMalloc(&dG.p, (size_t)n * DD * 8));
    HIPCHK(hipMalloc(&dd2.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&dstate.p, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dadj.p, (size_t)n * nw * 8));
    if (out.pair_d2) HIPCHK(hipMalloc(&dpair.p, (size_t)n * n * 8));
    HIPCHK(hipMalloc(&ddeg.p, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dbest.p, sizeof(unsigned long long)));
    HIPCHK(hipMalloc(&dclq.p, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dres.p, 2 * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dorder.p, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dF.p, (size_t)(kkD * kkD) * 8));
    HIPCHK(hipMalloc(&drows.p, (size_t)(D * kkD) * 8));
    HIPCHK(hipMalloc(&dy.p, (size_t)kkD * 8));
    HIPCHK(hipMalloc(&dacc.p, (size_t)kk * sizeof(int32_t)));
    HIPCHK(hipMalloc(&djd2.p, (size_t)kk * 8));
    HIPCHK(hipMalloc(&dnacc.p, sizeof(int32_t)));
    HIPCHK(hipMemsetAsync(dadj.p, 0, (size_t)n * nw * 8, s));
    if (out.pair_d2) HIPCHK(hipMemsetAsync(dpair.p, 0xff, (size_t)n * n * 8, s));   // NaN
    HIPCHK(hipMemsetAsync(dclq.p, 0xff, (size_t)n * sizeof(int32_t), s));           // -1
    HIPCHK(hipMemsetAsync(dacc.p, 0xff, (size_t)kk * sizeof(int32_t), s));
    HIPCHK(hipMemsetAsync(djd2.p, 0xff, (size_t)kk * 8, s));
    HIPCHK(hipMemsetAsync(dnacc.p, 0, sizeof(int32_t), s));
    EventTimer t_pair, t_clique, t_verify;
    hipError_t tail_err = hipSuccess;
    const auto note = [&](hipError_t e) { if (tail_err == hipSuccess) tail_err = e; };
    const CovTail tail = [&](hipStream_t st, const GraphBufs &gb, const double *joint) {
        CompatArgs a{};
        a.arena = gb.dev.arena; a.vpo = gb.dev.vpo;
        a.va = (const int32_t *)dca.p; a.vb = (const int32_t *)dcb.p; a.sa = (const int32_t *)dsa.p; a.sb = (const int32_t *)dsb.p;
        a.rec = (const double *)drec.p; a.joint = joint; a.ld = ld;
        a.U = (double *)dU.p; a.w = (double *)dw.p; a.z = (double *)dz.p; a.M = (double *)dM.p; a.G = (double *)dG.p;
        a.d2 = (double *)dd2.p; a.state = (int32_t *)dstate.p; a.adj = (unsigned long long *)dadj.p; a.nw = nw;
        a.pair_d2 = (double *)dpair.p; a.n = n; a.max_d2 = max_d2; a.pair_max_d2 = pair_max_d2;
        VerifyArgs v{};
        v.U = a.U; v.w = a.w; v.M = a.M; v.d2 = a.d2; v.sa = a.sa; v.sb = a.sb; v.joint = joint; v.ld = ld;
        v.clique = (const int32_t *)dclq.p; v.res = (const int32_t *)dres.p; v.order = (int32_t *)dorder.p; v.state = a.state;
        v.F = (double *)dF.p; v.rows = (double *)drows.p; v.y = (double *)dy.p; v.jmax = (const double *)djmax.p;
        v.acc = (int32_t *)dacc.p; v.jd2 = (double *)djd2.p; v.nacc = (int32_t *)dnacc.p; v.kk = kk;
        note(t_pair.start(st));
        by_dim(D, [&](auto d) {
            hipLaunchKernelGGL((sp_compat_init_kernel<decltype(d)::value>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, a);
            hipLaunchKernelGGL((sp_compat_pair_kernel<decltype(d)::value>), dim3((unsigned)nw, (unsigned)((n + kCompatTileI - 1) / kCompatTileI)), dim3(256), 0,
                               st, a);
        });
        note(t_pair.stop(st));
        note(t_clique.start(st));
        launch_clique(st, a.adj, n, nw, a.state, (int32_t *)ddeg.p, (unsigned long long *)dbest.p, (int32_t *)dclq.p, (int32_t *)dres.p);
        note(t_clique.stop(st));
        note(t_verify.start(st));
        by_dim(D, [&](auto d) { hipLaunchKernelGGL((sp_compat_verify_kernel<decltype(d)::value>), dim3(1), dim3(256), 0, st, v); });
        note(t_verify.stop(st));
    };
    if ((rc = cov_solve_device(s, in, va, vb, dst, ld, nblk, joint_len, djoint, stats.solve, err, errlen, &tail))) return rc;
    HIPCHK(tail_err);
    float ms0 = 0, ms1 = 0, ms2 = 0;
    HIPCHK(t_pair.ms(ms0));
    HIPCHK(t_clique.ms(ms1));
    HIPCHK(t_verify.ms(ms2));
    int32_t res[2] = {0, -1}, nacc = 0;
    std::vector<int32_t> deg((size_t)n), state((size_t)n);
    HIPCHK(hipMemcpy(res, dres.p, sizeof res, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&nacc, dnacc.p, sizeof nacc, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(deg.data(), ddeg.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(state.data(), dstate.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out.compatible, dacc.p, (size_t)kk * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out.joint_d2, djd2.p, (size_t)kk * 8, hipMemcpyDeviceToHost));
    if (out.clique) HIPCHK(hipMemcpy(out.clique, dclq.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out.d2) HIPCHK(hipMemcpy(out.d2, dd2.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (out.pair_d2) HIPCHK(hipMemcpy(out.pair_d2, dpair.p, (size_t)n * n * 8, hipMemcpyDeviceToHost));
    if (out.degree) std::copy(deg.begin(), deg.end(), out.degree);
    if (out.status) std::copy(state.begin(), state.end(), out.status);
    int64_t twice = 0;
    int eligible = 0;
    for (int i = 0; i < n; i++) {
        twice += deg[i];
        eligible += state[i] != SPG_CAND_INFO_NOT_PD && state[i] != SPG_CAND_GATED;
    }
    *ncompat = nacc;
    stats.eligible = eligible;
    stats.consistent_pairs = twice / 2;
    stats.clique_size = res[0];
    stats.seed = res[1];
    stats.pair_seconds = 1e-3 * ms0;
    stats.clique_seconds = 1e-3 * ms1;
    stats.verify_seconds = 1e-3 * ms2;
    return 0;
}

}  // namespace spg
