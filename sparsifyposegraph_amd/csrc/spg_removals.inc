// csrc/spg_removals.inc — the vertices to remove, chosen on the device by spatial redundancy (spg_graph_select_removals;
// DESIGN 5g-V). Included at the end of spg_sparse.inc, after spg_propose.inc: the grid (pp_key_kernel, pp_insert_kernel,
// pp_scan_kernel, pp_scatter_kernel through pp_stage_grid / pp_sort_cells), pp_dist, pp_angle, pp_runs and pp_entry are
// those of the proposal. Nothing of them is edited.
//
// A vertex is named by its rank in ascending id order; pos[rank] is its place in the total order of the header (the forced
// vertices first). The kept set is the lexicographically first maximal independent set of the relation "redundant with" in
// that order:
//   rm_init_kernel     state per rank (forced: kept, else undecided), the first worklist = the unforced ranks in order
//   rm_decide_kernel   one wavefront per undecided vertex of the worklist; relaunched by the host until the list is empty
//   rm_flag_kernel     1 per removed rank; pp_scan_kernel over it gives every removed vertex its place in ascending id
//   rm_list_kernel     the removed ranks, compacted
//   rm_rep_kernel      one wavefront per removed vertex: its representative, the kept redundant vertex of smallest (dist, id)
// The invariant. The verdict of v is a function of the verdicts of its redundant neighbours EARLIER in the order alone:
// removed iff one of them is kept, kept iff all of them are removed. A state word goes from undecided to kept or to removed
// once and never changes again. rm_decide_kernel reads and writes the words in place, without any ordering between
// workgroups: a read that misses a verdict written in the same launch sees "undecided" and so only postpones v to the next
// launch; it can never produce a different verdict. The earliest undecided vertex of a launch has every earlier neighbour
// decided before the launch began, so every launch decides at least that one and the loop ends after at most n launches.
// The outputs therefore depend neither on the order of the worklist nor on the order of its atomics (an integer counter);
// rounds and pairs_tested may. No workgroup waits for another, no cooperative launch, no floating-point atomics.

namespace {

constexpr int kRmUndecided = 0, kRmKept = 1, kRmRemoved = 2;

struct RmArgs {
    PpArgs g;                      // the grid and the cell-sorted arrays; radius and max_angle are read from here
    const uint32_t *pos;           // per rank: place in the order
    int n_forced;                  // places below this are the keep list
    int32_t *state;                // per rank
    const int32_t *work;           // the ranks to decide in this launch
    int32_t *next, *next_count;    // those it could not decide
    int n_work;
    unsigned long long *tested;    // distance evaluations
    int32_t *flag;                 // per rank: removed
    const int32_t *off;            // exclusive scan of flag
    int32_t *list;                 // the removed ranks, ascending
    int32_t *out_id, *out_rep;     // per removed vertex
    double *out_dist;
};

// two distinct vertices are redundant: rules 1 and 2 of the proposal, the angle asked in (lower rank, higher rank) order
template <int D>
__device__ __forceinline__ bool rm_redundant(const PpArgs &a, int ra, const double *pa, int rb, const double *pb, double &dist) {
    constexpr int DIM = D == 6 ? 3 : 2;
    dist = pp_dist<DIM>(pa, pb);
    if (!(dist <= a.radius)) return false;
    if (a.max_angle > 0.0) {
        const int lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
        if (!(pp_angle<D>(a.arena, a.vpo[lo], a.vpo[hi]) <= a.max_angle)) return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void rm_init_kernel(RmArgs a, int32_t *work) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.g.n) return;
    const int p = (int)a.pos[r];
    a.state[r] = p < a.n_forced ? kRmKept : kRmUndecided;
    if (p >= a.n_forced) work[p - a.n_forced] = r;
}

// One wavefront per undecided vertex v. Of the entries of its 3^dim cells only those earlier in the order matter, and of
// those only the ones not removed are measured: a kept one that is redundant removes v (the ballot ends the walk), an
// undecided one that is redundant leaves v undecided.
template <int D>
__global__ __launch_bounds__(64) void rm_decide_kernel(RmArgs a) {
    constexpr int DIM = D == 6 ? 3 : 2;
    __shared__ int rs[27], rp[28];
    const int lane = threadIdx.x, rv = a.work[blockIdx.x];
    const unsigned pv = a.pos[rv];
    double pa[3] = {0, 0, 0};
    {
        const double *p = a.g.arena + a.g.vpo[rv];
        for (int k = 0; k < DIM; k++) pa[k] = p[k];
    }
    const int total = pp_runs<DIM>(a.g, rv, lane, rs, rp);
    bool removed = false, pending = false;
    unsigned long long tested = 0;
    for (int t0 = 0; t0 < total && !removed; t0 += 64) {
        const int t = t0 + lane;
        bool hit = false, wait = false, measured = false;
        if (t < total) {
            const int e = pp_entry<DIM>(rs, rp, t), rb = a.g.srank[e];
            if (rb != rv && a.pos[rb] < pv) {
                const int st = __hip_atomic_load(&a.state[rb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (st != kRmRemoved) {
                    const double pb[3] = {a.g.sx[e], a.g.sy[e], DIM == 3 ? a.g.sz[e] : 0.0};
                    double dist;
                    measured = true;
                    if (rm_redundant<D>(a.g, rv, pa, rb, pb, dist)) {
                        hit = st == kRmKept;
                        wait = st == kRmUndecided;
                    }
                }
            }
        }
        tested += __popcll(__ballot(measured));
        removed = __ballot(hit) != 0ull;
        pending = pending || __ballot(wait) != 0ull;
    }
    if (lane != 0) return;
    if (tested) atomicAdd(a.tested, tested);
    if (removed) __hip_atomic_store(&a.state[rv], kRmRemoved, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (!pending) __hip_atomic_store(&a.state[rv], kRmKept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else a.next[atomicAdd(a.next_count, 1)] = rv;
}

__global__ __launch_bounds__(256) void rm_flag_kernel(RmArgs a) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < a.g.n) a.flag[r] = a.state[r] == kRmRemoved;
}

__global__ __launch_bounds__(256) void rm_list_kernel(RmArgs a) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < a.g.n && a.flag[r]) a.list[a.off[r]] = r;
}

// One wavefront per removed vertex: the minimum of (dist, id) over the kept vertices redundant with it, lane by lane over
// the sweeps and then across the wavefront. Every removed vertex has one: the kept neighbour that removed it.
template <int D>
__global__ __launch_bounds__(64) void rm_rep_kernel(RmArgs a) {
    constexpr int DIM = D == 6 ? 3 : 2;
    __shared__ int rs[27], rp[28];
    const int lane = threadIdx.x, rv = a.list[blockIdx.x];
    double pa[3] = {0, 0, 0};
    {
        const double *p = a.g.arena + a.g.vpo[rv];
        for (int k = 0; k < DIM; k++) pa[k] = p[k];
    }
    const int total = pp_runs<DIM>(a.g, rv, lane, rs, rp);
    double bd = __builtin_inf();
    int bid = 0x7fffffff;
    for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        if (t < total) {
            const int e = pp_entry<DIM>(rs, rp, t), rb = a.g.srank[e];
            if (rb != rv && a.state[rb] == kRmKept) {
                const double pb[3] = {a.g.sx[e], a.g.sy[e], DIM == 3 ? a.g.sz[e] : 0.0};
                double dist;
                if (rm_redundant<D>(a.g, rv, pa, rb, pb, dist)) {
                    const int idb = a.g.id[rb];
                    if (pp_less(dist, idb, bd, bid)) { bd = dist; bid = idb; }
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double od = __shfl_xor(bd, d);
        const int oi = __shfl_xor(bid, d);
        if (pp_less(od, oi, bd, bid)) { bd = od; bid = oi; }
    }
    if (lane == 0) {
        a.out_id[blockIdx.x] = a.g.id[rv];
        a.out_rep[blockIdx.x] = bid;
        a.out_dist[blockIdx.x] = bd;
    }
}

}  // namespace

namespace spg {

int hip_select_removals(void *stream, const RemovalsIn &in, bool fill, std::vector<int32_t> &removed, std::vector<int32_t> &representative,
                        std::vector<double> &rep_dist, spg_removal_stats &stats, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    const int n = in.n, D = in.D, n_free = in.n - in.n_forced;
    const char *what = "spg_graph_select_removals";
    int rc = 0;
    PpGrid G;
    RmArgs a{};
    if ((rc = pp_stage_grid(s, D, n, in.dev_arena, in.vpo, in.id, in.radius, "radius", in.table_bits, what, G, a.g, err, errlen))) return rc;
    a.g.max_angle = in.max_angle;
    DevBuf dpos, dstate, dwork[2], dcount, dtested, dflag, doff, dlist, doid, dorep, dodist;
    if ((rc = upload(dpos, in.pos, (size_t)n, s))) {
        snprintf(err, errlen, "%s: staging the order failed (%d)", what, rc);
        return rc;
    }
    HIPCHK(hipMalloc(&dstate.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&dwork[0].p, (size_t)std::max(n_free, 1) * 4));
    HIPCHK(hipMalloc(&dwork[1].p, (size_t)std::max(n_free, 1) * 4));
    HIPCHK(hipMalloc(&dcount.p, 4));
    HIPCHK(hipMalloc(&dtested.p, 8));
    HIPCHK(hipMalloc(&dflag.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&doff.p, ((size_t)n + 1) * 4));
    HIPCHK(hipMemsetAsync(dtested.p, 0, 8, s));
    a.pos = (const uint32_t *)dpos.p; a.n_forced = in.n_forced; a.state = (int32_t *)dstate.p; a.next_count = (int32_t *)dcount.p;
    a.tested = (unsigned long long *)dtested.p; a.flag = (int32_t *)dflag.p; a.off = (const int32_t *)doff.p;
    const dim3 per_vertex((unsigned)((n + 255) / 256));
    EventTimer t_decide, t_out;
    float ms1 = 0, ms2 = 0;
    HIPCHK(t_decide.start(s));
    pp_sort_cells(s, D, n, G, a.g);
    hipLaunchKernelGGL(rm_init_kernel, per_vertex, dim3(256), 0, s, a, (int32_t *)dwork[0].p);
    HIPCHK(hipGetLastError());
    // one launch per round; the size of the next worklist is the only thing read back
    int n_work = n_free, rounds = 0;
    for (int cur = 0; n_work > 0; cur ^= 1) {
        a.work = (const int32_t *)dwork[cur].p; a.next = (int32_t *)dwork[cur ^ 1].p; a.n_work = n_work;
        HIPCHK(hipMemsetAsync(dcount.p, 0, 4, s));
        by_dim(D, [&](auto d) { hipLaunchKernelGGL((rm_decide_kernel<decltype(d)::value>), dim3((unsigned)n_work), dim3(64), 0, s, a); });
        HIPCHK(hipGetLastError());
        int32_t left = 0;
        HIPCHK(hipMemcpyAsync(&left, dcount.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        rounds++;
        if (left < 0 || left >= n_work) {   // every launch decides its earliest vertex
            snprintf(err, errlen, "%s: round %d left %d of %d vertices undecided", what, rounds, (int)left, n_work);
            return SPG_EHIP;
        }
        n_work = left;
    }
    long long *stat = (long long *)G.dstat.p;
    hipLaunchKernelGGL(rm_flag_kernel, per_vertex, dim3(256), 0, s, a);
    hipLaunchKernelGGL((pp_scan_kernel<int32_t>), dim3(1), dim3(1024), 0, s, (const int32_t *)dflag.p, n, (int32_t *)doff.p, stat + 3);
    HIPCHK(hipGetLastError());
    HIPCHK(t_decide.stop(s));
    long long hstat[6];
    unsigned long long tested = 0;
    HIPCHK(hipMemcpyAsync(hstat, G.dstat.p, sizeof hstat, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&tested, dtested.p, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(t_decide.ms(ms1));
    const long long total = hstat[3];
    stats.n_cells = (int32_t)hstat[2];
    stats.max_cell_population = (int32_t)hstat[1];
    stats.table_slots = (int64_t)G.slots;
    stats.n_live = n; stats.n_forced = in.n_forced;
    stats.n_removed = (int32_t)total; stats.n_kept = (int32_t)(n - total);
    stats.rounds = rounds;
    stats.pairs_tested = (int64_t)tested;
    stats.device_seconds = 1e-3 * (G.ms + ms1);
    removed.clear(); representative.clear(); rep_dist.clear();
    if (!fill || total == 0) return 0;
    HIPCHK(hipMalloc(&dlist.p, (size_t)total * 4));
    HIPCHK(hipMalloc(&doid.p, (size_t)total * 4));
    HIPCHK(hipMalloc(&dorep.p, (size_t)total * 4));
    HIPCHK(hipMalloc(&dodist.p, (size_t)total * 8));
    a.list = (int32_t *)dlist.p; a.out_id = (int32_t *)doid.p; a.out_rep = (int32_t *)dorep.p; a.out_dist = (double *)dodist.p;
    HIPCHK(t_out.start(s));
    hipLaunchKernelGGL(rm_list_kernel, per_vertex, dim3(256), 0, s, a);
    by_dim(D, [&](auto d) { hipLaunchKernelGGL((rm_rep_kernel<decltype(d)::value>), dim3((unsigned)total), dim3(64), 0, s, a); });
    HIPCHK(hipGetLastError());
    HIPCHK(t_out.stop(s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(t_out.ms(ms2));
    stats.device_seconds += 1e-3 * ms2;
    removed.resize((size_t)total); representative.resize((size_t)total); rep_dist.resize((size_t)total);
    HIPCHK(hipMemcpy(removed.data(), doid.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(representative.data(), dorep.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(rep_dist.data(), dodist.p, (size_t)total * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace spg
