// csrc/spg_propose.inc — loop-closure candidates proposed on the device (spg_graph_propose_candidates; DESIGN 5g-N).
// Included at the end of spg_sparse.inc, after spg_compat.inc: sp_relative_kernel, cov_solve_device and the host helpers
// are those of the relative covariances. Nothing of them is edited.
//
// Stage A, a fixed-radius neighbour search over the translations of the live vertices. A vertex is named by its rank in
// ascending id order, so rank order is id order. A uniform grid with cell edge = search_radius lives in an open-addressing
// hash table of 64-bit cell keys (21 bits per axis):
//   pp_key_kernel      cell key per vertex, non-finite poses and cell coordinates that do not fit are flagged
//   pp_insert_kernel   keys into the table by 64-bit compare-and-swap, population per cell by integer atomics
//   pp_scan_kernel     exclusive scan (one workgroup), here over the table's populations
//   pp_scatter_kernel  ranks and positions into cell-sorted SoA arrays: a cell is one contiguous run
//   pp_tau_kernel      pass 1: per query vertex the m-th smallest (dist, id) of its qualifying partners, tau
//   pp_pair_kernel     pass 2: per vertex a the kept partners b of higher rank; counts, then (after a scan over the
//                      vertices) fills them and sorts the vertex's segment by rank
//   pp_emit_kernel     ids, dist and angle of every kept pair
// The order inside a cell depends on the order of the scatter's atomics; no result does: tau is the m-th element of a
// total order, the counts are sums of integers, and every vertex's segment is sorted before it is read. No floating-point
// atomics anywhere.
// Passes 1 and 2 are one wavefront per vertex (a 64-thread workgroup): the runs of the vertex's 3^dim cells are laid end
// to end and walked 64 entries at a time with coalesced reads, so a cell of hundreds of poses costs its wavefront a few
// sweeps instead of serialising 63 idle lanes behind one, and a sparse neighbourhood (the usual ten partners) is one sweep.
// Stage B (pp_gate_kernel): the range statistic of every kept pair from the rel / cov of sp_relative_kernel, on the device.
// The host staging of the grid (pp_stage_grid, pp_sort_cells) is shared with spg_removals.inc, which is included after this
// file and walks the same cells.

namespace {

constexpr unsigned long long kPpEmpty = ~0ull;   // no cell key: 63 bits are used
constexpr int kPpBias = 1 << 20;                 // cell coordinates in [-2^20, 2^20)
constexpr int kPpScanPer = 8;                    // items per thread and sweep of pp_scan_kernel

struct PpArgs {
    const double *arena;
    const int64_t *vpo;          // per rank: pose offset in the arena
    const int32_t *id;           // per rank, ascending
    const uint8_t *isq;          // per rank: the vertex is a query
    const int32_t *qlist;        // ranks of the queries
    const int32_t *adjptr, *adj; // CSR of the live adjacency over ranks, rows ascending
    int n;
    double radius, max_angle;
    int min_gap, m;
    unsigned long long *tkey;    // the table: cell key, population, start of the run
    int32_t *tcnt, *tstart, *tfill;
    unsigned mask;               // slots - 1
    unsigned long long *vkey;    // per rank: cell key and slot
    int32_t *vslot;
    int32_t *srank;              // cell-sorted: rank and position
    double *sx, *sy, *sz;
    double *tau_d;               // per rank: tau = (dist, id); (-inf, -1) for a vertex that is no query
    int32_t *tau_id;
    int32_t *cnt;                // per rank: kept partners of higher rank
    const long long *off;        // their exclusive scan
    int32_t *oa, *ob;            // per kept pair: ranks
    unsigned long long *ctr;     // [0] pairs_tested, [1] n_qualifying
    int32_t *flag;               // [0] lowest rank with a non-finite pose, [1] with a cell that does not fit, [2] the table is full
    int32_t *ij;                 // outputs per kept pair
    double *dist, *angle;
    long long total;
};

__device__ __forceinline__ unsigned pp_hash(unsigned long long k) {
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return (unsigned)k;
}

// slot of a cell key or -1; a table without an empty slot is walked once round
__device__ __forceinline__ int pp_find(const unsigned long long *tkey, unsigned mask, unsigned long long key) {
    unsigned h = pp_hash(key) & mask;
    for (unsigned probe = 0; probe <= mask; probe++) {
        const unsigned long long k = tkey[h];
        if (k == key) return (int)h;
        if (k == kPpEmpty) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

// (d0, i0) < (d1, i1)
__device__ __forceinline__ bool pp_less(double d0, int i0, double d1, int i1) { return d0 < d1 || (d0 == d1 && i0 < i1); }

// || pa - pb ||: every product and sum rounded on its own, so that the value does not depend on the kernel it is inlined
// into or on which of the two vertices asks
template <int DIM>
__device__ __forceinline__ double pp_dist(const double *pa, const double *pb) {
#pragma clang fp contract(off)
    const double dx = pa[0] - pb[0], dy = pa[1] - pb[1];
    double s = dx * dx + dy * dy;
    if (DIM == 3) {
        const double dz = pa[2] - pb[2];
        s = s + dz * dz;
    }
    return sqrt(s);
}

// rotation angle of Xa^-1 Xb through the device geometry: | wrap(theta_b - theta_a) |, or 2 atan2(|vec|, |w|) of the
// quaternion of Ra^T Rb
template <int D>
__device__ __forceinline__ double pp_angle(const double *arena, long long oa, long long ob) {
    if (D == 6) {
        double Xa[kIso], Xb[kIso], Z[kIso], q[4];
        iso_from_tq(arena + oa, Xa);
        iso_from_tq(arena + ob, Xb);
        iso_inv_mul(Xa, Xb, Z);
        R_to_quat(Z, q);
        return 2.0 * atan2(sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), fabs(q[3]));
    }
    return fabs(normalize_theta(arena[ob + 2] - arena[oa + 2]));
}

// rules 1 to 4 for two distinct vertices; the angle and the adjacency are asked in (lower rank, higher rank) order
template <int D>
__device__ __forceinline__ bool pp_qualify(const PpArgs &a, int ra, const double *pa, int rb, const double *pb, double &dist) {
    constexpr int DIM = D == 6 ? 3 : 2;
    dist = pp_dist<DIM>(pa, pb);
    if (!(dist <= a.radius)) return false;
    const int lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
    if (a.min_gap > 1 && (long long)a.id[hi] - (long long)a.id[lo] < (long long)a.min_gap) return false;
    if (a.max_angle > 0.0 && !(pp_angle<D>(a.arena, a.vpo[lo], a.vpo[hi]) <= a.max_angle)) return false;
    int l = a.adjptr[lo], r = a.adjptr[lo + 1];
    while (l < r) {
        const int mid = (l + r) >> 1, v = a.adj[mid];
        if (v == hi) return false;
        if (v < hi) l = mid + 1; else r = mid;
    }
    return true;
}

template <int D>
__global__ __launch_bounds__(256) void pp_key_kernel(PpArgs a) {
    constexpr int DIM = D == 6 ? 3 : 2, PS = D == 6 ? 7 : 3;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n) return;
    const double *p = a.arena + a.vpo[r];
    bool finite = true;
    for (int k = 0; k < PS; k++) finite = finite && isfinite(p[k]);
    a.tau_d[r] = -__builtin_inf();
    a.tau_id[r] = -1;
    if (!finite) { atomicMin(&a.flag[0], r); a.vkey[r] = kPpEmpty; return; }
    unsigned long long key = 0;
    bool fits = true;
    for (int k = 0; k < DIM; k++) {
        const double c = floor(p[k] / a.radius);
        fits = fits && c >= -(double)kPpBias && c < (double)kPpBias;
        if (fits) key |= (unsigned long long)((long long)c + kPpBias) << (21 * k);
    }
    if (!fits) { atomicMin(&a.flag[1], r); key = kPpEmpty; }
    a.vkey[r] = key;
}

__global__ __launch_bounds__(256) void pp_insert_kernel(PpArgs a) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n) return;
    const unsigned long long key = a.vkey[r];
    unsigned h = pp_hash(key) & a.mask;
    for (unsigned probe = 0; probe <= a.mask; probe++) {
        const unsigned long long prev = atomicCAS(&a.tkey[h], kPpEmpty, key);
        if (prev == kPpEmpty || prev == key) {
            a.vslot[r] = (int32_t)h;
            atomicAdd(&a.tcnt[h], 1);
            return;
        }
        h = (h + 1) & a.mask;
    }
    a.vslot[r] = -1;
    atomicExch(&a.flag[2], 1);
}

// off[0 .. n] = exclusive scan of cnt[0 .. n) in one workgroup of 1024; stat = {total, largest entry, entries above zero}
template <class T>
__global__ __launch_bounds__(1024) void pp_scan_kernel(const int32_t *cnt, int n, T *off, long long *stat) {
    __shared__ long long wsum[16];
    __shared__ int smax, snz;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) { smax = 0; snz = 0; }
    __syncthreads();
    long long carry = 0;
    int mx = 0, nz = 0;
    for (long long base = 0; base < n; base += 1024 * kPpScanPer) {
        const long long i0 = base + (long long)tid * kPpScanPer;
        int v[kPpScanPer];
        long long s = 0;
#pragma unroll
        for (int j = 0; j < kPpScanPer; j++) {
            v[j] = i0 + j < n ? cnt[i0 + j] : 0;
            s += v[j];
            mx = v[j] > mx ? v[j] : mx;
            nz += v[j] > 0;
        }
        long long inc = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        __syncthreads();   // wsum of the sweep before has been read
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        long long before = carry + inc - s, all = 0;
        for (int k = 0; k < 16; k++) {
            if (k < w) before += wsum[k];
            all += wsum[k];
        }
#pragma unroll
        for (int j = 0; j < kPpScanPer; j++) {
            if (i0 + j < n) off[i0 + j] = (T)before;
            before += v[j];
        }
        carry += all;
    }
    atomicMax(&smax, mx);
    atomicAdd(&snz, nz);
    __syncthreads();
    if (tid == 0) {
        off[n] = (T)carry;
        stat[0] = carry; stat[1] = smax; stat[2] = snz;
    }
}

template <int D>
__global__ __launch_bounds__(256) void pp_scatter_kernel(PpArgs a) {
    constexpr int DIM = D == 6 ? 3 : 2;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n) return;
    const int slot = a.vslot[r];
    const int pos = a.tstart[slot] + atomicAdd(&a.tfill[slot], 1);
    const double *p = a.arena + a.vpo[r];
    a.srank[pos] = r;
    a.sx[pos] = p[0];
    a.sy[pos] = p[1];
    if (DIM == 3) a.sz[pos] = p[2];
}

// The runs of the 3^DIM cells around vertex r, laid end to end: rs[c] = start of run c in the cell-sorted arrays,
// rp[c] = entries before it; returns the total. One wavefront; rs / rp: 27 / 28 ints of LDS.
template <int DIM>
__device__ __forceinline__ int pp_runs(const PpArgs &a, int r, int lane, int *rs, int *rp) {
    constexpr int NC = DIM == 3 ? 27 : 9;
    int start = 0, len = 0;
    if (lane < NC) {
        const unsigned long long key = a.vkey[r];
        unsigned long long nk = 0;
        bool ok = true;
        int c = lane;
        for (int k = 0; k < DIM; k++) {
            const int v = (int)((key >> (21 * k)) & 0x1fffff) + (c % 3) - 1;
            c /= 3;
            ok = ok && v >= 0 && v < 2 * kPpBias;
            nk |= (unsigned long long)(unsigned)v << (21 * k);
        }
        const int slot = ok ? pp_find(a.tkey, a.mask, nk) : -1;
        if (slot >= 0) { start = a.tstart[slot]; len = a.tcnt[slot]; }
    }
    int inc = len;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane < NC) { rs[lane] = start; rp[lane] = inc - len; }
    if (lane == NC - 1) rp[NC] = inc;
    __syncthreads();
    return rp[NC];
}

// entry t of the laid-out runs -> index into the cell-sorted arrays
template <int DIM>
__device__ __forceinline__ int pp_entry(const int *rs, const int *rp, int t) {
    constexpr int NC = DIM == 3 ? 27 : 9;
    int c = 0;
#pragma unroll
    for (int k = 1; k < NC; k++) c += rp[k] <= t;
    return rs[c] + (t - rp[c]);
}

// Pass 1, one wavefront per query vertex: tau = the m-th smallest (dist, id) of its qualifying partners, (+inf, INT_MAX)
// with fewer than m of them or m = 0. The m smallest so far sit sorted in lanes 0 .. m - 1; a sweep's candidates below
// the current m-th are inserted one at a time (the lanes above the insertion point shift up by one).
template <int D>
__global__ __launch_bounds__(64) void pp_tau_kernel(PpArgs a) {
    constexpr int DIM = D == 6 ? 3 : 2;
    __shared__ int rs[27], rp[28];
    const int lane = threadIdx.x, ra = a.qlist[blockIdx.x], m = a.m;
    double pa[3] = {0, 0, 0};
    {
        const double *p = a.arena + a.vpo[ra];
        for (int k = 0; k < DIM; k++) pa[k] = p[k];
    }
    const int total = pp_runs<DIM>(a, ra, lane, rs, rp);
    double ld = __builtin_inf();
    int lid = 0x7fffffff;
    unsigned long long tested = 0;
    for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        bool q = false, other = false;
        double dist = 0;
        int idb = 0;
        if (t < total) {
            const int e = pp_entry<DIM>(rs, rp, t), rb = a.srank[e];
            other = rb != ra;
            if (other) {
                const double pb[3] = {a.sx[e], a.sy[e], DIM == 3 ? a.sz[e] : 0.0};
                q = pp_qualify<D>(a, ra, pa, rb, pb, dist);
                idb = a.id[rb];
            }
        }
        tested += __popcll(__ballot(other));
        if (m > 0) {
            const double td = __shfl(ld, m - 1);
            const int ti = __shfl(lid, m - 1);
            unsigned long long todo = __ballot(q && pp_less(dist, idb, td, ti));
            while (todo) {
                const int j = __builtin_ctzll(todo);
                todo &= todo - 1;
                const double nd = __shfl(dist, j);
                const int ni = __shfl(idb, j);
                if (!pp_less(nd, ni, __shfl(ld, m - 1), __shfl(lid, m - 1))) continue;
                const bool above = pp_less(nd, ni, ld, lid);
                const double ud = __shfl_up(ld, 1);
                const int ui = __shfl_up(lid, 1);
                const int uabove = __shfl_up((int)above, 1);
                if (above) {
                    if (lane > 0 && uabove) { ld = ud; lid = ui; }
                    else { ld = nd; lid = ni; }
                }
            }
        }
    }
    const double td = m > 0 ? __shfl(ld, m - 1) : __builtin_inf();
    const int ti = m > 0 ? __shfl(lid, m - 1) : 0x7fffffff;
    if (lane == 0) {
        a.tau_d[ra] = td;
        a.tau_id[ra] = ti;
        if (tested) atomicAdd(&a.ctr[0], tested);
    }
}

// Pass 2, one wavefront per vertex a: its partners b of higher rank that qualify (rules 1 to 5) and are kept under tau_a or
// tau_b. FILL = false: cnt[a] and the number qualifying. FILL = true: the kept ranks into ob[off[a] ..) in sweep order,
// then the segment sorted ascending in place (a bitonic network whose exchanges all put the smaller value first, so the
// positions beyond the segment stand for +inf and are never touched).
template <int D, bool FILL>
__global__ __launch_bounds__(64) void pp_pair_kernel(PpArgs a) {
    constexpr int DIM = D == 6 ? 3 : 2;
    __shared__ int rs[27], rp[28];
    const int lane = threadIdx.x, ra = blockIdx.x;
    double pa[3] = {0, 0, 0};
    {
        const double *p = a.arena + a.vpo[ra];
        for (int k = 0; k < DIM; k++) pa[k] = p[k];
    }
    const int total = pp_runs<DIM>(a, ra, lane, rs, rp);
    const bool qa = a.isq[ra] != 0;
    const double tda = a.tau_d[ra];
    const int tia = a.tau_id[ra], ida = a.id[ra];
    const long long base = FILL ? a.off[ra] : 0;
    int nk = 0;
    unsigned long long nq = 0;
    for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        bool qual = false, keep = false;
        int rb = -1;
        if (t < total) {
            const int e = pp_entry<DIM>(rs, rp, t);
            rb = a.srank[e];
            if (rb > ra) {
                const bool qb = a.isq[rb] != 0;
                if (qa || qb) {
                    const double pb[3] = {a.sx[e], a.sy[e], DIM == 3 ? a.sz[e] : 0.0};
                    double dist;
                    qual = pp_qualify<D>(a, ra, pa, rb, pb, dist);
                    if (qual)
                        keep = (qa && !pp_less(tda, tia, dist, a.id[rb])) || (qb && !pp_less(a.tau_d[rb], a.tau_id[rb], dist, ida));
                }
            }
        }
        const unsigned long long km = __ballot(keep);
        nq += __popcll(__ballot(qual));
        if (FILL && keep) {
            const long long pos = base + nk + __popcll(km & ((1ull << lane) - 1ull));
            a.ob[pos] = rb;
            a.oa[pos] = ra;
        }
        nk += __popcll(km);
    }
    if (!FILL) {
        if (lane == 0) {
            a.cnt[ra] = nk;
            if (nq) atomicAdd(&a.ctr[1], nq);
        }
        return;
    }
    if (nk < 2) return;
    int32_t *x = a.ob + base;
    int P = 2;
    while (P < nk) P <<= 1;
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            __syncthreads();   // the exchanges of the step before (and the fill) are visible to the wavefront
            const bool flip = stride == (size >> 1);
            for (int i = lane; i < (P >> 1); i += 64) {
                const int blk = i / stride, j = i - blk * stride;
                const int l = blk * 2 * stride + j, h = flip ? blk * 2 * stride + 2 * stride - 1 - j : l + stride;
                if (h < nk) {
                    const int xl = x[l], xh = x[h];
                    if (xl > xh) { x[l] = xh; x[h] = xl; }
                }
            }
        }
    }
}

template <int D>
__global__ __launch_bounds__(256) void pp_emit_kernel(PpArgs a) {
    constexpr int DIM = D == 6 ? 3 : 2;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.total) return;
    const int ra = a.oa[p], rb = a.ob[p];
    const long long oa = a.vpo[ra], ob = a.vpo[rb];
    a.ij[2 * p] = a.id[ra];
    a.ij[2 * p + 1] = a.id[rb];
    a.dist[p] = pp_dist<DIM>(a.arena + oa, a.arena + ob);
    a.angle[p] = pp_angle<D>(a.arena, oa, ob);
}

// Stage B, one lane per kept pair: from z = rel (the current relative pose) and P = cov of sp_relative_kernel,
// rho = |t_z|, u = R_z^T t_z / rho (the direction of the range in the coordinates of the error's translation part),
// sigma^2 = u^T P_tt u, zscore = (rho - range) / sigma; sigma = 0: -inf when rho <= range, else +inf.
template <int D>
__global__ __launch_bounds__(256) void pp_gate_kernel(const double *rel, const double *cov, int n, double range, double *sigma, double *zscore) {
    constexpr int DIM = D == 6 ? 3 : 2, PS = D == 6 ? 7 : 3;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double *z = rel + (long long)i * PS, *P = cov + (long long)i * D * D;
    double t[3] = {z[0], z[1], DIM == 3 ? z[2] : 0.0}, u[3] = {1.0, 0.0, 0.0};
    const double rho = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    if (rho > 0.0) {
        if (D == 6) {
            double R[9];
            quat_to_R(z + 3, R);
            for (int j = 0; j < 3; j++) u[j] = (R[j] * t[0] + R[3 + j] * t[1] + R[6 + j] * t[2]) / rho;
        } else {
            const double c = cos(z[2]), s = sin(z[2]);
            u[0] = (c * t[0] + s * t[1]) / rho;
            u[1] = (-s * t[0] + c * t[1]) / rho;
        }
    }
    double s2 = 0;
    for (int r = 0; r < DIM; r++)
        for (int c = 0; c < DIM; c++) s2 += u[r] * P[r * D + c] * u[c];
    const double sg = s2 > 0.0 ? sqrt(s2) : 0.0, diff = rho - range;
    sigma[i] = sg;
    zscore[i] = sg > 0.0 ? diff / sg : (diff <= 0.0 ? -__builtin_inf() : __builtin_inf());
}

// The grid of a fixed-radius search over the n live vertices, staged once for every caller (the proposal, and the
// selection of removals in spg_removals.inc): the buffers of the table and of the cell-sorted arrays, the keys and their
// insertion, and the three refusals read back from the flags. `ms`: HIP-event time of the two kernels.
struct PpGrid {
    DevBuf dvpo, did, dtkey, dtcnt, dtstart, dtfill, dvkey, dvslot, dsrank, dsx, dsy, dsz, dtaud, dtaui, dflag, dstat;
    size_t slots = 0;
    float ms = 0;
};

// Fills the grid part of `a` (arena, vpo, id, n, radius, the table, the per-rank and the cell-sorted arrays, flag) and runs
// pp_key_kernel and pp_insert_kernel: nothing searches before every pose is known to have a cell. table_bits < 0:
// 2^ceil(log2(2 n)) slots. radius_name: what the caller's header calls the cell edge. G.dstat: 6 words for pp_scan_kernel.
int pp_stage_grid(hipStream_t s, int D, int n, const void *dev_arena, const int64_t *vpo, const int32_t *id, double radius, const char *radius_name,
                  int table_bits, const char *what, PpGrid &G, PpArgs &a, char *err, size_t errlen) {
    int bits = table_bits;
    if (bits < 0) for (bits = 1; (1ll << bits) < 2ll * n; bits++) {}
    const size_t slots = (size_t)1 << bits;
    G.slots = slots;
    int rc = 0;
    if ((rc = upload(G.dvpo, vpo, (size_t)n, s)) || (rc = upload(G.did, id, (size_t)n, s))) {
        snprintf(err, errlen, "%s: staging the vertices failed (%d)", what, rc);
        return rc;
    }
    HIPCHK(hipMalloc(&G.dtkey.p, slots * 8));
    HIPCHK(hipMalloc(&G.dtcnt.p, slots * 4));
    HIPCHK(hipMalloc(&G.dtstart.p, (slots + 1) * 4));
    HIPCHK(hipMalloc(&G.dtfill.p, slots * 4));
    HIPCHK(hipMalloc(&G.dvkey.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&G.dvslot.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&G.dsrank.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&G.dsx.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&G.dsy.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&G.dsz.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&G.dtaud.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&G.dtaui.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&G.dflag.p, 3 * 4));
    HIPCHK(hipMalloc(&G.dstat.p, 6 * 8));
    const int32_t flag0[3] = {0x7fffffff, 0x7fffffff, 0};
    HIPCHK(hipMemcpy(G.dflag.p, flag0, sizeof flag0, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(G.dtkey.p, 0xff, slots * 8, s));
    HIPCHK(hipMemsetAsync(G.dtcnt.p, 0, slots * 4, s));
    HIPCHK(hipMemsetAsync(G.dtfill.p, 0, slots * 4, s));
    a.arena = (const double *)dev_arena; a.vpo = (const int64_t *)G.dvpo.p; a.id = (const int32_t *)G.did.p;
    a.n = n; a.radius = radius;
    a.tkey = (unsigned long long *)G.dtkey.p; a.tcnt = (int32_t *)G.dtcnt.p; a.tstart = (int32_t *)G.dtstart.p; a.tfill = (int32_t *)G.dtfill.p;
    a.mask = (unsigned)(slots - 1);
    a.vkey = (unsigned long long *)G.dvkey.p; a.vslot = (int32_t *)G.dvslot.p; a.srank = (int32_t *)G.dsrank.p;
    a.sx = (double *)G.dsx.p; a.sy = (double *)G.dsy.p; a.sz = (double *)G.dsz.p; a.tau_d = (double *)G.dtaud.p; a.tau_id = (int32_t *)G.dtaui.p;
    a.flag = (int32_t *)G.dflag.p;
    const dim3 per_vertex((unsigned)((n + 255) / 256));
    EventTimer t_grid;
    HIPCHK(t_grid.start(s));
    by_dim(D, [&](auto d) { hipLaunchKernelGGL((pp_key_kernel<decltype(d)::value>), per_vertex, dim3(256), 0, s, a); });
    hipLaunchKernelGGL(pp_insert_kernel, per_vertex, dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(t_grid.stop(s));
    int32_t flag[3];
    HIPCHK(hipMemcpyAsync(flag, G.dflag.p, sizeof flag, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(t_grid.ms(G.ms));
    if (flag[0] != 0x7fffffff) {
        snprintf(err, errlen, "%s: the pose of vertex %d is not finite", what, (int)id[flag[0]]);
        return SPG_EINVAL;
    }
    if (flag[1] != 0x7fffffff) {
        snprintf(err, errlen, "%s: the cell coordinate of vertex %d does not fit 21 bits at %s %g", what, (int)id[flag[1]], radius_name, radius);
        return SPG_ECAPACITY;
    }
    if (flag[2]) {
        snprintf(err, errlen, "%s: a cell table of %lld slots is smaller than the number of occupied cells", what, (long long)slots);
        return SPG_ECAPACITY;
    }
    return 0;
}

// the cells as contiguous runs: the scan over the table's populations (its figures in G.dstat[0 .. 2]) and the scatter
void pp_sort_cells(hipStream_t s, int D, int n, PpGrid &G, const PpArgs &a) {
    hipLaunchKernelGGL((pp_scan_kernel<int32_t>), dim3(1), dim3(1024), 0, s, (const int32_t *)G.dtcnt.p, (int)G.slots, (int32_t *)G.dtstart.p,
                       (long long *)G.dstat.p);
    by_dim(D, [&](auto d) { hipLaunchKernelGGL((pp_scatter_kernel<decltype(d)::value>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a); });
}

}  // namespace

namespace spg {

int hip_propose_search(void *stream, const ProposeIn &in, bool fill, std::vector<int32_t> &ij, std::vector<double> &dist, std::vector<double> &angle,
                       spg_propose_stats &stats, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    const int n = in.n, D = in.D;
    const char *what = "spg_graph_propose_candidates";
    int rc = 0;
    PpGrid G;
    PpArgs a{};
    DevBuf disq, dq, daptr, dadj, dcnt, doff, doa, dob, dctr, dij, ddist, dangle;
    if ((rc = upload(disq, in.isq, (size_t)n, s)) || (rc = upload(dq, in.qlist, (size_t)in.nq, s)) || (rc = upload(daptr, in.adjptr, (size_t)n + 1, s)) ||
        (rc = upload(dadj, in.adj, (size_t)in.adjptr[n], s))) {
        snprintf(err, errlen, "%s: staging the vertices failed (%d)", what, rc);
        return rc;
    }
    HIPCHK(hipMalloc(&dcnt.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&doff.p, ((size_t)n + 1) * 8));
    HIPCHK(hipMalloc(&dctr.p, 2 * 8));
    HIPCHK(hipMemsetAsync(dctr.p, 0, 2 * 8, s));
    if ((rc = pp_stage_grid(s, D, n, in.dev_arena, in.vpo, in.id, in.radius, "search_radius", in.table_bits, what, G, a, err, errlen))) return rc;
    const size_t slots = G.slots;
    a.isq = (const uint8_t *)disq.p; a.qlist = (const int32_t *)dq.p; a.adjptr = (const int32_t *)daptr.p; a.adj = (const int32_t *)dadj.p;
    a.max_angle = in.max_angle; a.min_gap = in.min_id_gap; a.m = in.m;
    a.cnt = (int32_t *)dcnt.p; a.off = (const long long *)doff.p; a.ctr = (unsigned long long *)dctr.p;
    EventTimer t_search, t_fill;
    float ms1 = 0, ms2 = 0;
    const float ms0 = G.ms;
    HIPCHK(t_search.start(s));
    long long *stat = (long long *)G.dstat.p;
    pp_sort_cells(s, D, n, G, a);
    by_dim(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        if (in.nq > 0) hipLaunchKernelGGL((pp_tau_kernel<DD>), dim3((unsigned)in.nq), dim3(64), 0, s, a);
        hipLaunchKernelGGL((pp_pair_kernel<DD, false>), dim3((unsigned)n), dim3(64), 0, s, a);
    });
    hipLaunchKernelGGL((pp_scan_kernel<long long>), dim3(1), dim3(1024), 0, s, (const int32_t *)dcnt.p, n, (long long *)doff.p, stat + 3);
    HIPCHK(hipGetLastError());
    HIPCHK(t_search.stop(s));
    long long hstat[6];
    unsigned long long hctr[2];
    HIPCHK(hipMemcpyAsync(hstat, G.dstat.p, sizeof hstat, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hctr, dctr.p, sizeof hctr, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(t_search.ms(ms1));
    const long long total = hstat[3];
    stats.n_cells = (int32_t)hstat[2];
    stats.max_cell_population = (int32_t)hstat[1];
    stats.table_slots = (int64_t)slots;
    stats.pairs_tested = (int64_t)hctr[0];
    stats.n_qualifying = (int64_t)hctr[1];
    stats.n_kept = total;
    stats.device_seconds = 1e-3 * (ms0 + ms1);
    if (total > 0x7fffffffll) {
        snprintf(err, errlen, "%s: %lld pairs kept, limited to 2^31 - 1", what, total);
        return SPG_ECAPACITY;
    }
    ij.clear(); dist.clear(); angle.clear();
    if (!fill || total == 0) return 0;
    HIPCHK(hipMalloc(&doa.p, (size_t)total * 4));
    HIPCHK(hipMalloc(&dob.p, (size_t)total * 4));
    HIPCHK(hipMalloc(&dij.p, (size_t)total * 8));
    HIPCHK(hipMalloc(&ddist.p, (size_t)total * 8));
    HIPCHK(hipMalloc(&dangle.p, (size_t)total * 8));
    a.oa = (int32_t *)doa.p; a.ob = (int32_t *)dob.p; a.ij = (int32_t *)dij.p; a.dist = (double *)ddist.p; a.angle = (double *)dangle.p;
    a.total = total;
    HIPCHK(t_fill.start(s));
    by_dim(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        hipLaunchKernelGGL((pp_pair_kernel<DD, true>), dim3((unsigned)n), dim3(64), 0, s, a);
        hipLaunchKernelGGL((pp_emit_kernel<DD>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(t_fill.stop(s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(t_fill.ms(ms2));
    stats.device_seconds += 1e-3 * ms2;
    ij.resize((size_t)total * 2); dist.resize((size_t)total); angle.resize((size_t)total);
    HIPCHK(hipMemcpy(ij.data(), dij.p, (size_t)total * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dist.data(), ddist.p, (size_t)total * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(angle.data(), dangle.p, (size_t)total * 8, hipMemcpyDeviceToHost));
    return 0;
}

// Stage B: hip_sparse_relative at the current relative pose with rel and cov left on the device, where pp_gate_kernel
// reads them; only sigma and zscore cross to the host.
int hip_propose_gate(void *stream, const DenseGraphIn &in, const int32_t *va, const int32_t *vb, const int64_t *dst, int32_t ld, int64_t nblk,
                     int64_t blocks_len, const int32_t *ca, const int32_t *cb, const int32_t *slot, int n, double range, double *sigma, double *zscore,
                     spg_cov_solve_stats &stats, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    const int D = in.D, PS = D == 6 ? 7 : 3;
    int rc = 0;
    DevBuf dblocks, dca, dcb, dslot, drel, dcov, dsig, dz;
    if ((rc = upload(dca, ca, (size_t)n, s)) || (rc = upload(dcb, cb, (size_t)n, s)) || (rc = upload(dslot, slot, (size_t)n, s))) {
        snprintf(err, errlen, "staging the pairs failed (%d)", rc);
        return rc;
    }
    HIPCHK(hipMalloc(&drel.p, (size_t)n * PS * 8));
    HIPCHK(hipMalloc(&dcov.p, (size_t)n * D * D * 8));
    HIPCHK(hipMalloc(&dsig.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&dz.p, (size_t)n * 8));
    const CovTail tail = [&](hipStream_t st, const GraphBufs &gb, const double *blocks) {
        const RelArgs ra{gb.dev.arena, gb.dev.vpo, (const int32_t *)dca.p, (const int32_t *)dcb.p, (const int32_t *)dslot.p, nullptr, blocks,
                         (double *)drel.p, (double *)dcov.p, nullptr, nullptr, n};
        by_dim(D, [&](auto d) {
            constexpr int DD = decltype(d)::value;
            hipLaunchKernelGGL((sp_relative_kernel<DD>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, ra);
            hipLaunchKernelGGL((pp_gate_kernel<DD>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double *)drel.p, (const double *)dcov.p, n,
                               range, (double *)dsig.p, (double *)dz.p);
        });
    };
    if ((rc = cov_solve_device(s, in, va, vb, dst, ld, nblk, blocks_len, dblocks, stats, err, errlen, &tail))) return rc;
    HIPCHK(hipMemcpy(sigma, dsig.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(zscore, dz.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace spg
