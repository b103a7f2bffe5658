// csrc/spg_init.inc — chordal initialisation of the pose estimates on the device (included by spg_dense.hip after
// spg_sparse.inc, whose solver it drives). DESIGN.md 5k; the equations are stated at spg_graph_initialize in include/spg.h.
//
// Reference: none in the reference project, which always starts from file poses. The method is the chordal relaxation
// of Carlone et al. 2015 (GTSAM's InitializePose3) restricted to scalar weights; the spanning-tree mode (host,
// spg_host_global.cpp) is g2o's computeInitialGuess with unit costs and supplies the orientation of degenerate vertices.
//
// Two symmetric positive-definite systems with 3 x 3 blocks on the pattern of the binary edges, both over ONE plan of
// the multifrontal solver (block size 3 whatever the pose dimension):
//   rotations     diagonal (sum kappa) I, block (b, a) = -kappa G_e, right-hand sides from the fixed vertex — three columns
//                 for SE3 (G = R_ab^T, unknown R_i^T), one for SE2 embedded as (cos, sin, 0) (G = Rz(theta_ab));
//   translations  the tau-weighted graph Laplacian (x) I, one right-hand side built with the projected rotations.
// Everything gathers per vertex over the incident-edge CSR in ascending edge order: no atomics, same input same bits.
namespace {

// kappa_e (mode 0) or tau_e (mode 1) of a binary edge record: the mean of the diagonal of the rotation / translation
// block of Omega (upper triangle row-wise after the measurement, translation block first)
template <int GD>
__device__ __forceinline__ double init_edge_weight(const double *rec, int mode) {
    constexpr int PS = (GD == 6) ? 7 : 3;
    auto dg = [&](int i) { return rec[PS + i * GD - i * (i - 1) / 2]; };
    if (GD == 6) return mode == 0 ? (dg(3) + dg(4) + dg(5)) / 3.0 : (dg(0) + dg(1) + dg(2)) / 3.0;
    return mode == 0 ? dg(2) : (dg(0) + dg(1)) / 2.0;
}

__device__ __forceinline__ void rot_z(double th, double *R) {
    const double c = cos(th), s = sin(th);
    R[0] = c; R[1] = -s; R[2] = 0; R[3] = s; R[4] = c; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1;
}

// One wavefront per free vertex v, lanes < 9 own entry (r, c) of a 3 x 3 block: the lower block triangle and the
// diagonal block of v's block row through `sink` (the interface of dense_assemble_kernel's sinks), and v's rows of the
// right-hand sides. mode 0: rotations, rhs column c at rhs + c * nvec (SE2: column 0 only). mode 1: translations,
// rot = the projected rotations (10 doubles per vertex, init_project_kernel), one right-hand side.
// g.pos = 3 * elimination position of a free vertex, -1 otherwise; fixed_v is the only live vertex that is not free.
template <int GD, class Sink>
__global__ __launch_bounds__(64) void init_assemble_kernel(GraphDev g, Sink sink, int mode, int fixed_v, const double *rot, double *rhs, int nvec) {
    constexpr int PS = (GD == 6) ? 7 : 3;
    __shared__ double G[9], Mf[9];
    const int v = blockIdx.x, tid = threadIdx.x;
    const int pv = g.pos[v];
    if (pv < 0) return;
    const int r = tid / 3, c = tid - 3 * r;
    const bool act = tid < 9;
    if (tid == 0) {
        const double *pf = g.arena + g.vpo[fixed_v];
        if (mode == 0) {
            if (GD == 6) {   // M_f = R_f^T
                double R[9];
                quat_to_R(pf + 3, R);
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int k = 0; k < 3; k++) Mf[i * 3 + k] = R[k * 3 + i];
            } else {
                rot_z(pf[2], Mf);   // column 0 = (cos, sin, 0)
            }
        } else {
            Mf[0] = pf[0]; Mf[1] = pf[1]; Mf[2] = (GD == 6) ? pf[2] : 0.0;
        }
    }
    __syncthreads();
    double diag = 0, racc = 0;
    for (int ii = g.rowptr[v]; ii < g.rowptr[v + 1]; ii++) {
        const int e = g.inc[ii];
        const spg_edge_ref er = g.er[e];
        if (er.kind != SPG_EDGE_BINARY) continue;
        const int vi = g.ev[er.vbegin], vj = g.ev[er.vbegin + 1];
        if (vi == vj) continue;
        const double *rec = g.arena + er.off;
        const double w = init_edge_weight<GD>(rec, mode);
        const int u = (v == vi) ? vj : vi, pu = g.pos[u];
        const bool head = v == vj;   // v is the edge's second vertex b: block (v, u) = -w G, else -w G^T
        if (mode == 0) {
            if (tid == 0) {
                if (GD == 6) {
                    double R[9];
                    quat_to_R(rec + 3, R);
#pragma unroll
                    for (int i = 0; i < 3; i++)
#pragma unroll
                        for (int k = 0; k < 3; k++) G[i * 3 + k] = R[k * 3 + i];
                } else {
                    rot_z(rec[2], G);
                }
            }
            __syncthreads();
            if (act) {
                if (r == c) diag += w;
                if (pu >= 0) {
                    if (pu < pv) sink.add(pv, pu, r, c, -w * (head ? G[r * 3 + c] : G[c * 3 + r]));
                } else {
                    double s = 0;
#pragma unroll
                    for (int k = 0; k < 3; k++) s += (head ? G[r * 3 + k] : G[k * 3 + r]) * Mf[k * 3 + c];
                    racc += w * s;
                }
            }
            __syncthreads();
        } else {
            if (act) {
                if (r == c) diag += w;
                if (pu >= 0 && pu < pv) sink.add(pv, pu, r, c, (r == c) ? -w : 0.0);
            }
            if (tid < 3) {
                // R_a t_ab with a = the edge's first vertex
                const double *Ra = rot + 10ll * vi + 3 * tid;
                const double d = Ra[0] * rec[0] + Ra[1] * rec[1] + ((GD == 6) ? Ra[2] * rec[2] : 0.0);
                racc += head ? w * d : -(w * d);
                if (pu < 0) racc += w * Mf[tid];
            }
        }
    }
    if (act) sink.diag(pv, r, c, (r == c) ? diag : 0.0);
    if (mode == 0) {
        if (act && (GD == 6 || c == 0)) rhs[(long long)c * nvec + pv + r] = racc;
    } else if (tid < 3) {
        rhs[pv + tid] = racc;
    }
    sink.finish(v, tid);
}

// Cyclic Jacobi on a symmetric 3 x 3 matrix held in registers: a = (a00, a01, a02, a11, a12, a22) ends (nearly)
// diagonal, V (row-major) holds the eigenvectors in its columns.
__device__ __forceinline__ void jacobi_rot3(double &app, double &aqq, double &apq, double &arp, double &arq, double *V, int p, int q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
    app -= t * apq; aqq += t * apq; apq = 0.0;
    const double xp = arp, xq = arq;
    arp = cs * xp - sn * xq; arq = sn * xp + cs * xq;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double vp = V[i * 3 + p], vq = V[i * 3 + q];
        V[i * 3 + p] = cs * vp - sn * vq; V[i * 3 + q] = sn * vp + cs * vq;
    }
}

// Nearest rotation to M (row-major): U diag(1, 1, det(U V^T)) V^T of M = U S V^T, from the eigenvectors of M^T M:
// u1 = M v1 / s1, u2 = M v2 / s2, and the third column u1 x u2 with the sign that makes the product proper — which is
// what the diag(...) factor does to U's third column. Returns the second-largest singular value; below ~1e-8 s1 it is
// rounding noise, which is why the caller's threshold (1e-6) is the rule and not zero. R is unset when it is 0.
__device__ __forceinline__ double project_rotation(const double *M, double *R) {
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a00 += M[k * 3] * M[k * 3]; a01 += M[k * 3] * M[k * 3 + 1]; a02 += M[k * 3] * M[k * 3 + 2];
        a11 += M[k * 3 + 1] * M[k * 3 + 1]; a12 += M[k * 3 + 1] * M[k * 3 + 2]; a22 += M[k * 3 + 2] * M[k * 3 + 2];
    }
    double V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int sweep = 0; sweep < 12; sweep++) {
        const double off = fabs(a01) + fabs(a02) + fabs(a12);
        if (off <= 1e-30 * (fabs(a00) + fabs(a11) + fabs(a22)) || off == 0.0) break;
        jacobi_rot3(a00, a11, a01, a02, a12, V, 0, 1);
        jacobi_rot3(a00, a22, a02, a01, a12, V, 0, 2);
        jacobi_rot3(a11, a22, a12, a01, a02, V, 1, 2);
    }
    // columns of V by descending eigenvalue
    int i0 = 0, i1 = 1, i2 = 2;
    double l0 = a00, l1 = a11, l2 = a22;
    if (l1 > l0) { double t = l0; l0 = l1; l1 = t; int k = i0; i0 = i1; i1 = k; }
    if (l2 > l0) { double t = l0; l0 = l2; l2 = t; int k = i0; i0 = i2; i2 = k; }
    if (l2 > l1) { double t = l1; l1 = l2; l2 = t; int k = i1; i1 = i2; i2 = k; }
    const double s1 = sqrt(fmax(l0, 0.0)), s2 = sqrt(fmax(l1, 0.0));
    if (!(s2 > 0.0)) return 0.0;
    double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        v1[i] = (i0 == 0) ? V[i * 3] : (i0 == 1) ? V[i * 3 + 1] : V[i * 3 + 2];
        v2[i] = (i1 == 0) ? V[i * 3] : (i1 == 1) ? V[i * 3 + 1] : V[i * 3 + 2];
        v3[i] = (i2 == 0) ? V[i * 3] : (i2 == 1) ? V[i * 3 + 1] : V[i * 3 + 2];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        u1[i] = (M[i * 3] * v1[0] + M[i * 3 + 1] * v1[1] + M[i * 3 + 2] * v1[2]) / s1;
        u2[i] = (M[i * 3] * v2[0] + M[i * 3 + 1] * v2[1] + M[i * 3 + 2] * v2[2]) / s2;
    }
    // u2 against u1 (they are orthogonal up to rounding), unit length
    const double d12 = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
#pragma unroll
    for (int i = 0; i < 3; i++) u2[i] -= d12 * u1[i];
    const double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]), n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) { u1[i] /= n1; u2[i] /= n2; }
    const double detV = v1[0] * (v2[1] * v3[2] - v2[2] * v3[1]) - v1[1] * (v2[0] * v3[2] - v2[2] * v3[0]) + v1[2] * (v2[0] * v3[1] - v2[1] * v3[0]);
    const double sg = detV < 0 ? -1.0 : 1.0;
    u3[0] = sg * (u1[1] * u2[2] - u1[2] * u2[1]);
    u3[1] = sg * (u1[2] * u2[0] - u1[0] * u2[2]);
    u3[2] = sg * (u1[0] * u2[1] - u1[1] * u2[0]);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) R[i * 3 + k] = u1[i] * v1[k] + u2[i] * v2[k] + u3[i] * v3[k];
    return s2;
}

// One lane per vertex: rot[10 v ..] = R_v (row-major; SE2: Rz(theta_v) and theta_v in slot 9). The fixed vertex takes
// its stored pose; a free vertex the projection of its solved block (x: the solved right-hand sides of mode 0), or —
// degenerate[v] = 1 — the orientation of the spanning-tree pose tree[ps v ..] (indexed by vertex).
template <int GD>
__global__ void init_project_kernel(const double *arena, const int64_t *vpo, const int32_t *pos, int nv, int fixed_v, const double *x, int nvec,
                                    const double *tree, double *rot, int32_t *degenerate) {
    constexpr int PS = (GD == 6) ? 7 : 3;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const int pv = pos[v];
    if (pv < 0 && v != fixed_v) return;
    double *Rv = rot + 10ll * v;
    int deg = 0;
    if (GD == 6) {
        double R[9];
        if (v == fixed_v) quat_to_R(arena + vpo[v] + 3, R);
        else {
            double M[9], Rt[9];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) M[r * 3 + c] = x[(long long)c * nvec + pv + r];
            const double s2 = project_rotation(M, Rt);
            if (!(s2 >= 1e-6)) { deg = 1; quat_to_R(tree + (long long)PS * v + 3, R); }
            else {
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int c = 0; c < 3; c++) R[r * 3 + c] = Rt[c * 3 + r];
            }
        }
#pragma unroll
        for (int i = 0; i < 9; i++) Rv[i] = R[i];
        Rv[9] = 0;
    } else {
        double th;
        if (v == fixed_v) th = arena[vpo[v] + 2];
        else {
            const double m0 = x[pv], m1 = x[pv + 1];
            if (!(sqrt(m0 * m0 + m1 * m1) >= 1e-6)) { deg = 1; th = tree[(long long)PS * v + 2]; }
            else th = atan2(m1, m0);
        }
        rot_z(th, Rv);
        Rv[9] = th;
    }
    degenerate[v] = deg;
}

// One lane per free vertex: its pose into the arena — translation x[pos ..], orientation rot (SE3: unit quaternion, w >= 0)
template <int GD>
__global__ void init_write_kernel(double *arena, const int64_t *vpo, const int32_t *pos, int nv, const double *x, const double *rot) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv || pos[v] < 0) return;
    double *p = arena + vpo[v];
    const double *t = x + pos[v], *Rv = rot + 10ll * v;
    p[0] = t[0]; p[1] = t[1];
    if (GD == 6) {
        double R[9], q[4];
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = Rv[i];
        R_to_quat(R, q);
        p[2] = t[2]; p[3] = q[0]; p[4] = q[1]; p[5] = q[2]; p[6] = q[3];
    } else {
        p[2] = Rv[9];
    }
}

}  // namespace

namespace spg {

// in.pos >= 0: the free vertices (their order numbers the blocks), -1 otherwise; fixed_v: the fixed vertex (index);
// tree: the spanning-tree poses, in.nv * pose stride doubles indexed by vertex (host). On success the arena holds the
// new estimates of the free vertices; on any error it is untouched. out: degenerate is assigned, the rest added to.
int hip_chordal_init(void *stream, const DenseGraphIn &in_, int fixed_v, const double *tree, spg_init_stats &out, char *err, size_t errlen) {
    hipStream_t s = (hipStream_t)stream;
    const int GD = in_.D, PS = GD == 6 ? 7 : 3, ncol = GD == 6 ? 3 : 1;
    // blocks by ascending pos; the plan is that of the binary edges' pattern with 3 x 3 blocks
    std::vector<int32_t> blk((size_t)in_.nv, -1), pos((size_t)in_.nv, -1);
    int nb = 0;
    {
        std::vector<std::pair<int32_t, int32_t>> order;
        for (int v = 0; v < in_.nv; v++) if (in_.pos[v] >= 0) order.push_back({in_.pos[v], v});
        std::sort(order.begin(), order.end());
        for (auto &p : order) blk[p.second] = nb++;
    }
    if (nb == 0) { snprintf(err, errlen, "chordal initialisation: no free vertex"); return SPG_EINVAL; }
    std::vector<spg_edge_ref> bin;
    for (int e = 0; e < in_.ne; e++) if (in_.er[e].kind == SPG_EDGE_BINARY) bin.push_back(in_.er[e]);
    DenseGraphIn pat = in_;
    pat.er = bin.data(); pat.ne = (int)bin.size();
    sparse::BlockGraph bg;
    block_graph_of(pat, blk, nb, bg);
    sparse::Plan plan;
    sparse::build_plan(bg, 3, nullptr, sparse_leaf(3), plan);
    for (int v = 0; v < in_.nv; v++) if (blk[v] >= 0) pos[v] = 3 * plan.iperm[blk[v]];
    out.supernodes += plan.nsn; out.front_bytes += (double)plan.pool * 8; out.factor_flops += plan.flops;
    const int64_t pool_len = std::max<int64_t>(plan.pool, 1);
    auto sp = std::make_unique<SparseSolver>();
    int rc = sp->init(std::move(plan), false, err, errlen);
    if (rc) return rc;
    DenseGraphIn in = in_;
    in.pos = pos.data();
    GraphBufs gb;
    if ((rc = stage_graph(in, gb, s))) { snprintf(err, errlen, "staging the graph for the chordal initialisation failed (%d)", rc); return rc; }
    const int nvec = 3 * nb, nv = in.nv;
    DevBuf rhs, rot, dtree, deg, bad;
    if (hipMalloc(&rhs.p, (size_t)ncol * nvec * 8) != hipSuccess || hipMalloc(&rot.p, (size_t)nv * 10 * 8) != hipSuccess ||
        hipMalloc(&deg.p, (size_t)nv * 4) != hipSuccess || hipMalloc(&bad.p, 2 * sizeof(int)) != hipSuccess) {
        snprintf(err, errlen, "chordal initialisation: device allocation failed");
        return SPG_ENOMEM;
    }
    if ((rc = upload(dtree, tree, (size_t)nv * PS, s))) { snprintf(err, errlen, "chordal initialisation: uploading the tree poses failed (%d)", rc); return rc; }
    HIPCHK(hipMemsetAsync(bad.p, 0, 2 * sizeof(int), s));
    HIPCHK(hipMemsetAsync(deg.p, 0, (size_t)nv * 4, s));
    HIPCHK(hipMemsetAsync(rot.p, 0, (size_t)nv * 10 * 8, s));
    double *x = (double *)rhs.p;
    const FrontSink sink{sp->dev, (int *)bad.p + 1};
    auto system = [&](int mode, int cols) -> int {
        if (hipMemsetAsync(sp->pool.p, 0, (size_t)pool_len * 8, s) != hipSuccess) return SPG_EHIP;
        by_dim(GD, [&](auto d) {
            hipLaunchKernelGGL((init_assemble_kernel<decltype(d)::value, FrontSink>), dim3(nv), dim3(64), 0, s, gb.dev, sink, mode, fixed_v,
                               (const double *)rot.p, x, nvec);
        });
        sp->shift(s, 0.0, nullptr, 0);
        sp->factor(s, (int *)bad.p);
        for (int c = 0; c < cols; c++) sp->solve(s, x + (size_t)c * nvec);
        return 0;
    };
    EventTimer timer;
    HIPCHK(timer.start(s));
    if ((rc = system(0, ncol))) { snprintf(err, errlen, "chordal initialisation: clearing the fronts failed"); return rc; }
    by_dim(GD, [&](auto d) {
        hipLaunchKernelGGL((init_project_kernel<decltype(d)::value>), dim3((nv + 255) / 256), dim3(256), 0, s, gb.dev.arena, gb.dev.vpo, gb.dev.pos, nv, fixed_v,
                           (const double *)x, nvec, (const double *)dtree.p, (double *)rot.p, (int32_t *)deg.p);
    });
    if ((rc = system(1, 1))) { snprintf(err, errlen, "chordal initialisation: clearing the fronts failed"); return rc; }
    HIPCHK(hipGetLastError());
    HIPCHK(timer.stop(s));
    int h_bad[2] = {0, 0};
    std::vector<int32_t> h_deg((size_t)nv);
    HIPCHK(hipMemcpyAsync(h_bad, bad.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_deg.data(), deg.p, (size_t)nv * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0;
    HIPCHK(timer.ms(ms));
    if (h_bad[0]) { snprintf(err, errlen, "chordal initialisation: a system is not positive definite"); return SPG_ENOTPD; }
    if (h_bad[1]) { snprintf(err, errlen, "chordal initialisation: a block lies outside the fronts of the plan"); return SPG_ESTATE; }
    // only now do the estimates change
    by_dim(GD, [&](auto d) {
        hipLaunchKernelGGL((init_write_kernel<decltype(d)::value>), dim3((nv + 255) / 256), dim3(256), 0, s, (double *)const_cast<void *>(in.dev_arena),
                           gb.dev.vpo, gb.dev.pos, nv, (const double *)x, (const double *)rot.p);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    int ndeg = 0;
    for (int32_t f : h_deg) ndeg += f;
    out.degenerate = ndeg;
    out.device_seconds += 1e-3 * ms;
    return 0;
}

}  // namespace spg
