// csrc/spg_glc_tail.inc — GLC edge construction, textually included inside blanket_kernel right after
// the Schur complement when a.algorithm == SPG_ALG_GLC (M1 holds Lambda_t, n = D*k).
//
// Device twin of TopologyProviderGLC::topology / getEdge / glc_chol / posdef_pinv
// (src/topology_provider_glc.cpp:42-185), PseudoChowLiu::marginal / jointMarginal
// (src/pseudo_chow_liu.cpp:130-167) and GLCReparamBinary (src/glc_reparam_binary.hpp:35-127).
// One blanket yields up to k equally shaped small problems (root: d x d, tree pairs: 2d x 2d), which
// are advanced in lockstep by the batched Gauss-Jordan / Jacobi routines of spg_dev_la.hpp.
{
    double *G = mat + L.o_G;
    const int gld = L.gld, gstride = L.gstride, CNT = L.gCNT;
    double *Tb = G, *Jb = G + (size_t)CNT * gstride, *Vb = G + 2 * (size_t)CNT * gstride, *Wk = G + 3 * (size_t)CNT * gstride;
    double *gmeas = smem + L.o_gmeas, *gev = smem + L.o_gev, *gcs = smem + L.o_gcs, *gscr = smem + L.o_gscr;
    int *gperm = ints + L.i_gperm, *gdone = ints + L.i_gdone, *gmeta = ints + L.i_gmeta, *gverts = ints + L.i_gverts;
    // misc[3] = edges emitted, misc[4] = endpoints emitted, misc[5] = doubles emitted (packed offset)
    if (tid == 0) { misc[3] = 0; misc[4] = 0; misc[5] = 0; }
    T.sync();
    double *Ng = smem + L.o_Ng;      // n x D orthonormal gauge basis (SPG_FLAG_GLC_KLD only)

    // Per-blanket KLD of the emitted edges (SPG_FLAG_GLC_KLD), after the publish: the graph update does not wait for it.
    // src/logdet_function.cpp:119-133 at the GLC edges' information, by the gauge route of the NFR branch (no inverse of a
    // singular matrix, no eigen-decomposition): A = sum_e (W_e G_e)^T (W_e G_e) in emission order, C = Lambda_t + N^ N^^T,
    //     kld = 1/2 ( tr(C^-1 A) - log det(A + N^ N^^T) + log det C - (n - D) ).
    // M1 still holds Lambda_t (the tail above only reads it); M2, M3 and the batch buffers are free, the records are read
    // back from the arena. Not defined — NaN and SPG_INFO_GLC_KLD_SKIPPED — when a root edge was emitted, when the edges
    // carry other than n - D rows (the 1e-8 cut dropped an eigenvalue: A and Lambda_t no longer share a range), when
    // trace(C^-1) >= 5e4 (the NFR route's guard) or when a factorisation fails. Below two kept vertices there is nothing
    // to compare: NaN without the bit, as in the NFR branch; a blanket whose status is not SPG_OK keeps its words too.
    auto glc_kld_tail = [&]() {
        // a blanket that failed (status) or has nothing to compare (k < 2, no root edge) keeps NaN and its info word, but
        // its record is complete as well: every flagged exit ends in the final word
        const bool wanted = (status == SPG_OK) && !(k < 2 && !(info & SPG_INFO_GLC_ROOT_EDGE));
        const int ng = misc[3];
        bool defined = wanted && !(info & SPG_INFO_GLC_ROOT_EDGE);
        int rows = 0;
        for (int e = 0; e < ng; e++) rows += gmeta[3 * e + 1] / (D * gmeta[3 * e + 2]) - 1;
        if (rows != n - D) defined = false;
        double val = __builtin_nan("");
        if (tid == 0) misc[0] = 0;
        T.sync();
        double ldC = 0.0, trC = 0.0;
        if (defined) {
            gauge_basis_raw<D>(T, pose + m * PSZ, k, Ng);
            gauge_orthonormalise<D>(T, n, Ng, eT);
            gauge_regularised<D>(T, M1, ld, n, Ng, M3);
            // ---- C^-1 into M3, log det C, trace(C^-1)
            if (use_wave) {
                const bool ok_ = wave_spd_inverse(M3, ld, n, tid, 0.0, M3, ldC, trC);
                defined = ok_ && (misc[0] == 0);
                T.sync();
            } else {
                chol_lower<NT>(T, M3, n, ld, Sv);
                defined = (misc[0] == 0);
                T.sync();
                if (defined) {
                    ldC = chol_logdet<NT>(T, M3, n, ld);
                    tri_inverse_lower<NT>(T, M3, M2, n, ld, Sv);
                    gram_lower_inverse<NT>(T, M2, M3, n, ld);
                    double d_ = 0;
                    for (int i = tid; i < n; i += NT) d_ += M3[i * ld + i];
                    trC = T.sum(d_);
                }
            }
            if (!(trC < 5e4) || !isfinite(trC)) defined = false;
        }
        if (defined) {
            for (int it = tid; it < n * ld; it += NT) M2[it] = 0.0;
            T.sync();
            double trp = 0;
            int vp = 0;
            for (int e = 0; e < ng; e++) {
                const int q = gmeta[3 * e + 2], dq = D * q, re = gmeta[3 * e + 1] / dq - 1;
                const int *vl = gverts + vp;
                double *Aw = G + q * 2 * DD;      // re x dq, behind the Jacobians (<= 4 batch buffers: 2 n D + (n - D) n doubles)
                glc_edge_rows(arena + bd.new_off + gmeta[3 * e + 0], q, re, vl, G, Aw);
                for (int it = tid; it < dq * dq; it += NT) {
                    const int R = it / dq, Cc = it - R * dq;
                    double sacc = 0;
                    for (int p = 0; p < re; p++) sacc += Aw[p * dq + R] * Aw[p * dq + Cc];
                    M2[((vl[R / D] - m) * D + R % D) * ld + (vl[Cc / D] - m) * D + Cc % D] += sacc;
                }
                // tr(C^-1 A_e) = sum_p a_p C^-1 a_p^T over the rows a_p of W_e G_e
                for (int it = tid; it < re * dq; it += NT) {
                    const int p = it / dq, i = it - p * dq;
                    const double *ci = M3 + ((vl[i / D] - m) * D + i % D) * ld;
                    double sacc = 0;
                    for (int j = 0; j < dq; j++) sacc += ci[(vl[j / D] - m) * D + j % D] * Aw[p * dq + j];
                    trp += Aw[it] * sacc;
                }
                T.sync();
                vp += q;
            }
            const double tr = T.sum(trp);
            gauge_add<D>(T, M2, ld, n, Ng);
            double ldA = 0.0;
            if (use_wave) {
                const bool ok_ = wave_spd_logdet(M2, ld, n, tid, ldA);
                defined = ok_;
            } else {
                chol_lower<NT>(T, M2, n, ld);
                defined = (misc[0] == 0);
                T.sync();
                if (defined) ldA = chol_logdet<NT>(T, M2, n, ld);
            }
            if (defined) val = 0.5 * (tr - ldA + ldC - (double)(n - D));
        }
        if (wanted && !defined) info |= SPG_INFO_GLC_KLD_SKIPPED;
        // the record is complete: final word, after a release (include/spg.h)
        if (tid == 0) {
            orec[2] = val; orec[1] = (double)info;
            __threadfence_system();
            __hip_atomic_store(&orec[5], SPG_FINAL_WORD(a.tag), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    };

    auto finish_glc = [&]() {
        T.sync();
        if (tid == 0) {
            int ng = misc[3];
            orec[0] = (double)status; orec[1] = (double)info; orec[2] = kld; orec[3] = min_gap; orec[4] = (double)ng;
            int vp = 0;
            for (int e = 0; e < ng; e++) {
                orec[SPG_OUT_HDR + 4 * e + 0] = (double)SPG_EDGE_GLC;
                orec[SPG_OUT_HDR + 4 * e + 1] = (double)gmeta[3 * e + 0];
                orec[SPG_OUT_HDR + 4 * e + 2] = (double)gmeta[3 * e + 1];
                orec[SPG_OUT_HDR + 4 * e + 3] = (double)gmeta[3 * e + 2];
                for (int i = 0; i < gmeta[3 * e + 2]; i++, vp++)
                    orec[SPG_OUT_HDR + 4 * bd.n_new_max + vp] = (double)gverts[vp];
            }
        }
        __threadfence_system();
        T.sync();
        if (tid == 0) __hip_atomic_store(&orec[5], SPG_READY_WORD(a.tag), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        if (a.flags & SPG_FLAG_GLC_KLD) glc_kld_tail();
    };

    // Schur complement of Lambda_t onto the blocks keepb[0..nkeep) (ascending), others marginalised
    // (PseudoChowLiu::marginal). Result (s x s, s = nkeep*D) at out with leading dimension gld.
    auto schur_onto = [&](int nkeep, int kb0, int kb1, double *out) -> bool {
        const int s = nkeep * D, ko = k - nkeep, no = ko * D;
        auto oblock = [&](int oi) { int b = oi; if (b >= kb0) b++; if (nkeep == 2 && b >= kb1) b++; return b; };
        auto krow = [&](int c) { return ((c / D) == 0 ? kb0 : kb1) * D + (c % D); };
        if (no > 0) {
            int sh = ceil_log2(no);
            for (int it = tid; it < (no << sh); it += NT) {
                int i = it >> sh, j = it & ((1 << sh) - 1);
                if (j <= i) M2[i * ld + j] = M1[(oblock(i / D) * D + i % D) * ld + oblock(j / D) * D + j % D];
            }
            for (int it = tid; it < no * s; it += NT) {
                int i = it / s, c = it - i * s;
                M3[i * ld + c] = M1[(oblock(i / D) * D + i % D) * ld + krow(c)];
            }
            T.sync();
            chol_lower<NT>(T, M2, no, ld);
            if (misc[0]) return false;
            tri_solve_lower<NT>(T, M2, no, ld, M3, s, ld);
        }
        for (int it = tid; it < s * s; it += NT) {
            int r_ = it / s, c = it - r_ * s;
            if (r_ <= c) {
                double v = M1[krow(r_) * ld + krow(c)];
                for (int p = 0; p < no; p++) v -= M3[p * ld + r_] * M3[p * ld + c];
                out[r_ * gld + c] = v;
                out[c * gld + r_] = v;
            }
        }
        T.sync();
        return true;
    };

    // getEdge for `cnt` problems of q vertices each; vl[b*q + i] = kept-local vertex index.
    // Tb[b] holds the (symmetric) target information on entry. Emits into the arena + gmeta/gverts.
    auto get_edges = [&](int cnt, int q, const int *vl) -> int {
        const int s = q * D;
        int sh = ceil_log2(s);
        for (int it = tid; it < ((cnt * s) << sh); it += NT) {
            int bi = it >> sh, c = it & ((1 << sh) - 1);
            if (c < s) Jb[(size_t)(bi / s) * gstride + (bi % s) * gld + c] = 0.0;
        }
        T.sync();
        // measurement = reparametrize(vertices) and its Jacobian at that measurement
        for (int it = tid; it < cnt * q; it += NT) {
            int b = it / q, i = it - b * q;
            int v0 = m + vl[b * q], vi = m + vl[b * q + i];
            double Ji[DD], Jj[DD];
            double *ms = gmeas + b * s + i * D;
            double *Jm = Jb + (size_t)b * gstride;
            if (D == 6) {
                double Z[kIso], qv[4];
                if (i == 0) {
                    double Xz[kIso] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
                    const double *X0 = pose + v0 * PSZ;
#pragma unroll
                    for (int t_ = 0; t_ < kIso; t_++) Z[t_] = X0[t_];
                    se3_edge_jac(Xz, X0, Z, Ji, Jj, nullptr);
                } else {
                    iso_inv_mul(pose + v0 * PSZ, pose + vi * PSZ, Z);
                    se3_edge_jac(pose + v0 * PSZ, pose + vi * PSZ, Z, Ji, Jj, nullptr);
                }
                R_to_quat(Z, qv);
                ms[0] = Z[9]; ms[1] = Z[10]; ms[2] = Z[11]; ms[3] = qv[0]; ms[4] = qv[1]; ms[5] = qv[2];
            } else {
                double z[3], xz[3] = {0, 0, 0};
                const double *xa = (i == 0) ? xz : (pose + v0 * PSZ);
                se2_between(xa, pose + vi * PSZ, z);
                z[2] = normalize_theta(z[2]);
                se2_edge_jac(xa, pose + vi * PSZ, z, Ji, Jj, nullptr);
                ms[0] = z[0]; ms[1] = z[1]; ms[2] = z[2];
            }
#pragma unroll
            for (int r_ = 0; r_ < D; r_++)
#pragma unroll
                for (int c = 0; c < D; c++) {
                    if (i > 0) Jm[(i * D + r_) * gld + c] = Ji[r_ * D + c];
                    Jm[(i * D + r_) * gld + i * D + c] = Jj[r_ * D + c];
                }
        }
        T.sync();
        STAMP(45);  // get_edges: reparam + J staged
        gj_inverse_batch<NT>(T, Jb, cnt, s, gld, gstride, gscr);
        if (misc[0]) return (int)SPG_ST_NONFINITE;
        STAMP(46);  // get_edges: J inverse
        // Wk = T * invJ ; m2 = invJ^T * Wk (symmetrised) -> Tb
        for (int it = tid; it < ((cnt * s) << sh); it += NT) {
            int bi = it >> sh, c = it & ((1 << sh) - 1);
            if (c < s) {
                int b = bi / s, r_ = bi - b * s;
                const double *Tm = Tb + (size_t)b * gstride, *Ji_ = Jb + (size_t)b * gstride;
                double acc = 0;
                for (int p = 0; p < s; p++) acc += Tm[r_ * gld + p] * Ji_[p * gld + c];
                Wk[(size_t)b * gstride + r_ * gld + c] = acc;
            }
        }
        T.sync();
        for (int it = tid; it < ((cnt * s) << sh); it += NT) {
            int bi = it >> sh, c = it & ((1 << sh) - 1);
            int b = bi / s, r_ = bi - b * s;
            if (c < s && r_ <= c) {
                const double *Wm = Wk + (size_t)b * gstride, *Ji_ = Jb + (size_t)b * gstride;
                double a1 = 0, a2 = 0;
                for (int p = 0; p < s; p++) { a1 += Ji_[p * gld + r_] * Wm[p * gld + c]; a2 += Ji_[p * gld + c] * Wm[p * gld + r_]; }
                double v = 0.5 * (a1 + a2);
                Tb[(size_t)b * gstride + r_ * gld + c] = v;
                Tb[(size_t)b * gstride + c * gld + r_] = v;
            }
        }
        T.sync();
        STAMP(47);  // get_edges: M = invJ^T T invJ
        jacobi_batch<NT>(T, Tb, Vb, cnt, s, gld, gstride, gcs, gdone);
        if (misc[0]) return (int)SPG_ST_EIG_FAIL;
        STAMP(48);  // get_edges: eig
        for (int it = tid; it < cnt * s; it += NT) { int b = it / s, i = it - b * s; gev[it] = Tb[(size_t)b * gstride + i * gld + i]; }
        T.sync();
        for (int it = tid; it < cnt * s; it += NT) {
            int b = it / s, i = it - b * s;
            double ki = gev[it];
            int rk = 0;
            for (int j = 0; j < s; j++) { double kj = gev[b * s + j]; rk += (kj < ki) || (kj == ki && j < i); }
            gperm[b * s + rk] = i;
        }
        T.sync();
        if (tid == 0) {
            for (int b = 0; b < cnt; b++) {
                int i0 = 0;
                while (i0 < s && gev[b * s + gperm[b * s + i0]] < 1e-8) i0++;  // glc_eps, src/topology_provider_glc.cpp:18,67
                gdone[b] = i0;
                int r_ = s - i0;
                if (r_ > 0) {
                    int e = misc[3]++;
                    gmeta[3 * e + 0] = misc[5];
                    gmeta[3 * e + 1] = s + r_ * s;
                    gmeta[3 * e + 2] = q;
                    for (int i = 0; i < q; i++) gverts[misc[4]++] = m + vl[b * q + i];
                    misc[5] += s + r_ * s;
                    if (q == 1) info |= 0;  // root edges are flagged by the caller
                }
            }
        }
        T.sync();
        {
            // records: meas (s) + W (r x s), W[e][c] = V[c][perm[i0+e]] * sqrt(lambda)
            int e = misc[3];
            // walk emitted edges of this call backwards to find their slots
            int slot = e;
            for (int b = cnt - 1; b >= 0; b--) {
                int i0 = gdone[b], r_ = s - i0;
                if (r_ <= 0) continue;
                slot--;
                double *rec = arena + bd.new_off + gmeta[3 * slot + 0];
                for (int c = tid; c < s; c += NT) rec[c] = gmeas[b * s + c];
                for (int it = tid; it < r_ * s; it += NT) {
                    int e2 = it / s, c = it - e2 * s;
                    int col = gperm[b * s + i0 + e2];
                    rec[s + it] = Vb[(size_t)b * gstride + c * gld + col] * sqrt(gev[b * s + col]);
                }
            }
        }
        T.sync();
        return (int)SPG_OK;
    };

    if (k == 0) { finish_glc(); return; }
    const bool single = (a.topology == SPG_TOPO_DENSE) || k == 1;
    if (single) {
        for (int it = tid; it < n * n; it += NT) { int i = it / n, j = it - i * n; Tb[i * gld + j] = M1[i * ld + j]; }
        for (int i = tid; i < k; i += NT) comp[i] = i;
        T.sync();
        int st_ = get_edges(1, k, comp);
        if (st_ != SPG_OK) { status = st_; finish_glc(); return; }
        if (k == 1 && misc[3] > 0) info |= SPG_INFO_GLC_ROOT_EDGE;
        finish_glc();
        return;
    }
    STAMP(40);  // glc tail start
    {
        int st_ = chow_liu_tree(T);
        if (st_ != SPG_OK) { status = st_; finish_glc(); return; }
    }
    STAMP(41);  // chow-liu
    // ------------------------------------------------------------------------------------------------ fast path
    // Tree topology on a blanket whose tile one wavefront holds in registers (n <= 24): the same edges without an
    // eigen-decomposition. For a tree pair (a, b) with joint marginal [[jaa, jab],[jba, jbb]] the reference's conditional
    // target [[jaa, jab],[jba, jba pinv(jaa) jab]] is G^T G with G = [R^T | R^-1 jab], jaa = R R^T (Cholesky; pinv = inverse
    // for a positive definite jaa), so M = J^-T G^T G J^-1 = W^T W with W = G J^-1 — d rows, J^-1 from the 2 x 2 block-arrow
    // structure of the reparametrisation. The reference's W (sqrt(lambda) v^T over the eigenvalues >= 1e-8 of M,
    // src/topology_provider_glc.cpp:59-71) has the same W^T W provided all d non-zero eigenvalues of M — those of the d x d
    // matrix W W^T — pass the cut: checked per edge by trace((W W^T)^-1) < 1e8. The root's unary edge is absent whenever
    // trace(J00^-T rootInfo J00^-1) < 1e-8 (every eigenvalue of a PSD matrix is below its trace), which is the case for
    // blankets of relative measurements. Any guard that fails sends the blanket through the eigen route below instead.
    // Measured on the bench graph: 723k -> ~160k cycles per blanket (batched Jacobi alone was 284k).
    bool fast_done = false;
    if (use_wave && !(a.flags & SPG_FLAG_FORCE_EIG)) {
        fast_done = [&]() -> bool {
            const int cnt = k - 1, s2 = 2 * D;
            // ---- rest-block inverse + Schur complement onto `nk` kept blocks kb[] -> out (ldo); register-resident inverse
            auto marginal_onto = [&](int nk, int kb0, int kb1, double *out, int ldo) -> bool {
                const int sdim = nk * D, no = n - sdim;
                auto oblock = [&](int oi) { int b_ = oi; if (b_ >= kb0) b_++; if (nk == 2 && b_ >= kb1) b_++; return b_; };
                auto krow = [&](int c) { return ((c / D) == 0 ? kb0 : kb1) * D + (c % D); };
                if (no > 0) {
                    for (int it = tid; it < no * no; it += NT) {
                        int i = it / no, j = it - i * no;
                        M2[i * ld + j] = M1[(oblock(i / D) * D + i % D) * ld + oblock(j / D) * D + j % D];
                    }
                    for (int it = tid; it < no * sdim; it += NT) {
                        int i = it / sdim, c = it - i * sdim;
                        M3[i * ld + c] = M1[(oblock(i / D) * D + i % D) * ld + krow(c)];
                    }
                    T.sync();
                    double ldt_, trt_;
                    if (!wave_spd_inverse(M2, ld, no, tid, 0.0, M2, ldt_, trt_)) return false;
                    T.sync();
                    // Y = inv * B into the rows no.. of M3 (n <= 24: 2 no <= ... rows available: M3 has n rows, no + no <= 2n; use Vb scratch instead)
                    double *Y = Vb;   // no x sdim, leading dimension sdim (<= 18 x 12 = 216 doubles <= CNT * gstride for k >= 3; k == 2 has no rest)
                    for (int it = tid; it < no * sdim; it += NT) {
                        int i = it / sdim, c = it - i * sdim;
                        double acc = 0;
                        for (int p = 0; p < no; p++) acc += M2[i * ld + p] * M3[p * ld + c];
                        Y[it] = acc;
                    }
                    T.sync();
                    for (int it = tid; it < sdim * sdim; it += NT) {
                        int r_ = it / sdim, c = it - r_ * sdim;
                        if (r_ <= c) {
                            double v = M1[krow(r_) * ld + krow(c)];
                            for (int p = 0; p < no; p++) v -= M3[p * ld + r_] * Y[p * sdim + c];
                            out[r_ * ldo + c] = v;
                            out[c * ldo + r_] = v;
                        }
                    }
                } else {
                    for (int it = tid; it < sdim * sdim; it += NT) { int r_ = it / sdim, c = it - r_ * sdim; out[r_ * ldo + c] = M1[krow(r_) * ld + krow(c)]; }
                }
                T.sync();
                return true;
            };
            // ---- root: no unary edge iff trace(J00^-T rootInfo J00^-1) < 1e-8
            const int root = pairs[0];
            if (!marginal_onto(1, root, -1, Tb, gld)) return false;
            if (tid == 0) {
                double Ji[DD], Jj[DD], Ti[DD], A_[DD];
                const double *X0 = pose + (m + root) * PSZ;
                if (D == 6) {
                    double Xz[kIso] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, Z[kIso];
#pragma unroll
                    for (int t_ = 0; t_ < kIso; t_++) Z[t_] = X0[t_];
                    se3_edge_jac(Xz, X0, Z, Ji, Jj, nullptr);
                } else {
                    double xz[3] = {0, 0, 0}, z[3];
                    se2_between(xz, X0, z);
                    z[2] = normalize_theta(z[2]);
                    se2_edge_jac(xz, X0, z, Ji, Jj, nullptr);
                }
                bool okr = small_inverse<D>(Jj, Ti);
                // trace(Ti^T R Ti) = sum_{r,c} R[r][c] (Ti Ti^T)[r][c]
#pragma unroll
                for (int r_ = 0; r_ < D; r_++)
#pragma unroll
                    for (int c = 0; c < D; c++) {
                        double acc = 0;
#pragma unroll
                        for (int p = 0; p < D; p++) acc += Ti[r_ * D + p] * Ti[c * D + p];
                        A_[r_ * D + c] = acc;
                    }
                double tr = 0;
#pragma unroll
                for (int r_ = 0; r_ < D; r_++)
#pragma unroll
                    for (int c = 0; c < D; c++) tr += Tb[r_ * gld + c] * A_[r_ * D + c];
                cs[1] = (okr && tr < 1e-8) ? 1.0 : 0.0;
            }
            T.sync();
            if (cs[1] == 0.0) return false;
            // ---- joint marginals of the tree pairs -> Wk[b]
            for (int b = 0; b < cnt; b++)
                if (!marginal_onto(2, pairs[2 * b], pairs[2 * b + 1], Wk + (size_t)b * gstride, gld)) return false;
            // ---- per pair, three lanes: (0) R = chol(jaa), R^-1 ; (1) J00^-1 and the measurement of a ; (2) J10, J11^-1 and the relative measurement
            // buffers per pair: Jb[b]: Rinv | R | J00inv | J10 ; Vb[b]: J11inv | Gb | Wb | U ; Tb[b]: Wa | Q | meas(2 D)
            if (tid == 0) cs[1] = 1.0;
            T.sync();
            for (int it = tid; it < 3 * cnt; it += NT) {
                const int b = it / 3, role = it - b * 3;
                double *Bj = Jb + (size_t)b * gstride, *Bv = Vb + (size_t)b * gstride, *Bt = Tb + (size_t)b * gstride;
                const double *jm = Wk + (size_t)b * gstride;
                const int va = m + pairs[2 * b], vb = m + pairs[2 * b + 1];
                if (role == 0) {
                    double Ab[DD], Li[DD];
#pragma unroll
                    for (int r_ = 0; r_ < D; r_++)
#pragma unroll
                        for (int c = 0; c < D; c++) Ab[r_ * D + c] = jm[r_ * gld + c];
                    bool okc = chol_reg<D>(Ab);
                    double dmin = Ab[0], dmax = Ab[0];
#pragma unroll
                    for (int r_ = 1; r_ < D; r_++) { dmin = fmin(dmin, Ab[r_ * D + r_]); dmax = fmax(dmax, Ab[r_ * D + r_]); }
                    // pinv == inverse only when jaa is safely positive definite: cond(R)^2 far below 1 / (eps d)
                    if (!okc || !(dmin > 1e-6 * dmax)) cs[1] = 0.0;
                    // lower-triangular inverse of R
#pragma unroll
                    for (int c = 0; c < D; c++)
#pragma unroll
                        for (int i = 0; i < D; i++) {
                            if (i < c) Li[i * D + c] = 0.0;
                            else if (i == c) Li[i * D + c] = 1.0 / Ab[c * D + c];
                            else {
                                double acc = 0;
#pragma unroll
                                for (int q = 0; q < D; q++) if (q >= c && q < i) acc += Ab[i * D + q] * Li[q * D + c];
                                Li[i * D + c] = -acc / Ab[i * D + i];
                            }
                        }
#pragma unroll
                    for (int r_ = 0; r_ < D; r_++)
#pragma unroll
                        for (int c = 0; c < D; c++) { Bj[r_ * D + c] = Li[r_ * D + c]; Bj[DD + r_ * D + c] = (c <= r_) ? Ab[r_ * D + c] : 0.0; }
                } else {
                    double Ji[DD], Jj[DD], Ti[DD];
                    double *ms = Bt + 2 * DD + (role - 1) * D;
                    if (D == 6) {
                        double Z[kIso], qv[4];
                        if (role == 1) {
                            double Xz[kIso] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
                            const double *X0 = pose + va * PSZ;
#pragma unroll
                            for (int t_ = 0; t_ < kIso; t_++) Z[t_] = X0[t_];
                            se3_edge_jac(Xz, X0, Z, Ji, Jj, nullptr);
                        } else {
                            iso_inv_mul(pose + va * PSZ, pose + vb * PSZ, Z);
                            se3_edge_jac(pose + va * PSZ, pose + vb * PSZ, Z, Ji, Jj, nullptr);
                        }
                        R_to_quat(Z, qv);
                        ms[0] = Z[9]; ms[1] = Z[10]; ms[2] = Z[11]; ms[3] = qv[0]; ms[4] = qv[1]; ms[5] = qv[2];
                    } else {
                        double z[3], xz[3] = {0, 0, 0};
                        const double *xa = (role == 1) ? xz : (pose + va * PSZ);
                        const double *xb = (role == 1) ? (pose + va * PSZ) : (pose + vb * PSZ);
                        se2_between(xa, xb, z);
                        z[2] = normalize_theta(z[2]);
                        se2_edge_jac(xa, xb, z, Ji, Jj, nullptr);
                        ms[0] = z[0]; ms[1] = z[1]; ms[2] = z[2];
                    }
                    if (!small_inverse<D>(Jj, Ti)) cs[1] = 0.0;
                    if (role == 1) {
#pragma unroll
                        for (int t_ = 0; t_ < DD; t_++) Bj[2 * DD + t_] = Ti[t_];                  // J00^-1
                    } else {
#pragma unroll
                        for (int t_ = 0; t_ < DD; t_++) { Bj[3 * DD + t_] = Ji[t_]; Bv[t_] = Ti[t_]; }   // J10, J11^-1
                    }
                }
            }
            T.sync();
            if (cs[1] == 0.0) return false;
            // ---- Gb = R^-1 jab ; Wb = Gb J11^-1 ; U = R^T - Wb J10 ; Wa = U J00^-1   (cnt x D x D items each)
            auto stage = [&](int which) {
                for (int it = tid; it < cnt * DD; it += NT) {
                    const int b = it / DD, rc = it - b * DD, r_ = rc / D, c = rc - r_ * D;
                    double *Bj = Jb + (size_t)b * gstride, *Bv = Vb + (size_t)b * gstride, *Bt = Tb + (size_t)b * gstride;
                    const double *jm = Wk + (size_t)b * gstride;
                    double acc = 0;
                    if (which == 0) {
#pragma unroll
                        for (int p = 0; p < D; p++) acc += Bj[r_ * D + p] * jm[p * gld + D + c];
                        Bv[DD + rc] = acc;
                    } else if (which == 1) {
#pragma unroll
                        for (int p = 0; p < D; p++) acc += Bv[DD + r_ * D + p] * Bv[p * D + c];
                        Bv[2 * DD + rc] = acc;
                    } else if (which == 2) {
#pragma unroll
                        for (int p = 0; p < D; p++) acc += Bv[2 * DD + r_ * D + p] * Bj[3 * DD + p * D + c];
                        Bv[3 * DD + rc] = Bj[DD + c * D + r_] - acc;       // (R^T)[r][c] = R[c][r]
                    } else if (which == 3) {
#pragma unroll
                        for (int p = 0; p < D; p++) acc += Bv[3 * DD + r_ * D + p] * Bj[2 * DD + p * D + c];
                        Bt[rc] = acc;
                    } else {
                        // Q = Wa Wa^T + Wb Wb^T
#pragma unroll
                        for (int p = 0; p < D; p++) acc += Bt[r_ * D + p] * Bt[c * D + p] + Bv[2 * DD + r_ * D + p] * Bv[2 * DD + c * D + p];
                        Bt[DD + rc] = acc;
                    }
                }
                T.sync();
            };
            stage(0); stage(1); stage(2); stage(3); stage(4);
            // ---- every non-zero eigenvalue of M = W^T W (= eigenvalues of Q = W W^T) must pass the 1e-8 cut
            for (int b = tid; b < cnt; b += NT) {
                const double *Bt = Tb + (size_t)b * gstride;
                double Ab[DD], Xr[DD];
#pragma unroll
                for (int t_ = 0; t_ < DD; t_++) Ab[t_] = Bt[DD + t_];
                bool okq = chol_reg<D>(Ab);
                chol_inverse_reg<D>(Ab, Xr);
                double tr = 0;
#pragma unroll
                for (int r_ = 0; r_ < D; r_++) tr += Xr[r_ * D + r_];
                if (!okq || !(tr < 1e8)) cs[1] = 0.0;
            }
            T.sync();
            if (cs[1] == 0.0) return false;
            // ---- emit: one binary GLC edge per tree pair, r = D rows
            if (tid == 0) {
                for (int b = 0; b < cnt; b++) {
                    int e = misc[3]++;
                    gmeta[3 * e + 0] = misc[5];
                    gmeta[3 * e + 1] = s2 + D * s2;
                    gmeta[3 * e + 2] = 2;
                    gverts[misc[4]++] = m + pairs[2 * b];
                    gverts[misc[4]++] = m + pairs[2 * b + 1];
                    misc[5] += s2 + D * s2;
                }
            }
            T.sync();
            for (int it = tid; it < cnt * (s2 + D * s2); it += NT) {
                const int b = it / (s2 + D * s2), w_ = it - b * (s2 + D * s2);
                const double *Bv = Vb + (size_t)b * gstride, *Bt = Tb + (size_t)b * gstride;
                double *rec = arena + bd.new_off + gmeta[3 * b + 0];
                double v;
                if (w_ < s2) v = Bt[2 * DD + w_];
                else { const int e2 = (w_ - s2) / s2, c = (w_ - s2) - e2 * s2; v = (c < D) ? Bt[e2 * D + c] : Bv[2 * DD + e2 * D + (c - D)]; }
                rec[w_] = v;
            }
            T.sync();
            return true;
        }();
        if (fast_done) { STAMP(49); finish_glc(); return; }
        if (tid == 0) { misc[0] = 0; misc[3] = 0; misc[4] = 0; misc[5] = 0; }
        T.sync();
    }
    // root unary edge from the marginal of the first vertex of the first tree edge
    {
        int root = pairs[0];
        if (!schur_onto(1, root, -1, Tb)) { status = SPG_ST_MARGINAL_NOT_PD; finish_glc(); return; }
        if (tid == 0) comp[0] = root;
        T.sync();
        int st_ = get_edges(1, 1, comp);
        if (st_ != SPG_OK) { status = st_; finish_glc(); return; }
        if (misc[3] > 0) info |= SPG_INFO_GLC_ROOT_EDGE;
    }
    STAMP(42);  // root edge
    // joint marginals of the tree pairs -> Wk[b]
    for (int b = 0; b < k - 1; b++) {
        if (!schur_onto(2, pairs[2 * b], pairs[2 * b + 1], Wk + (size_t)b * gstride)) { status = SPG_ST_MARGINAL_NOT_PD; finish_glc(); return; }
    }
    STAMP(43);  // joint marginals
    // conditional targets [[jaa, jab],[jba, jba pinv(jaa) jab]] (upper-symmetrised)
    {
        const int cnt = k - 1, s = 2 * D;
        for (int it = tid; it < cnt * DD; it += NT) {
            int b = it / DD, rc = it - b * DD, r_ = rc / D, c = rc - r_ * D;
            Jb[(size_t)b * gstride + r_ * gld + c] = Wk[(size_t)b * gstride + r_ * gld + c];
        }
        T.sync();
        jacobi_batch<NT>(T, Jb, Vb, cnt, D, gld, gstride, gcs, gdone);
        if (misc[0]) { status = SPG_ST_EIG_FAIL; finish_glc(); return; }
        // b2 = pinv(jaa) into Vb rows D..2D-1, cols 0..D-1 ; tolerance eps * D * max|lambda|
        for (int it = tid; it < cnt * DD; it += NT) {
            int b = it / DD, rc = it - b * DD, r_ = rc / D, c = rc - r_ * D;
            const double *Em = Jb + (size_t)b * gstride, *Vm = Vb + (size_t)b * gstride;
            double mx = 0;
#pragma unroll
            for (int p = 0; p < D; p++) mx = fmax(mx, fabs(Em[p * gld + p]));
            double tol = 2.220446049250313e-16 * D * mx;
            double acc = 0;
#pragma unroll
            for (int p = 0; p < D; p++) { double lam = Em[p * gld + p]; if (lam > tol) acc += Vm[r_ * gld + p] * Vm[c * gld + p] / lam; }
            Vb[(size_t)b * gstride + (D + r_) * gld + c] = acc;
        }
        T.sync();
        // tmp = b2 * jab into Vb rows D.., cols D..
        for (int it = tid; it < cnt * DD; it += NT) {
            int b = it / DD, rc = it - b * DD, r_ = rc / D, c = rc - r_ * D;
            const double *Jm = Wk + (size_t)b * gstride, *Vm = Vb + (size_t)b * gstride;
            double acc = 0;
#pragma unroll
            for (int p = 0; p < D; p++) acc += Vm[(D + r_) * gld + p] * Jm[p * gld + D + c];
            Vb[(size_t)b * gstride + (D + r_) * gld + D + c] = acc;
        }
        T.sync();
        for (int it = tid; it < cnt * s * s; it += NT) {
            int b = it / (s * s), rc = it - b * s * s, r_ = rc / s, c = rc - r_ * s;
            if (r_ > c) continue;
            const double *Jm = Wk + (size_t)b * gstride, *Vm = Vb + (size_t)b * gstride;
            double v;
            if (r_ >= D) {  // m4 = jba * tmp
                v = 0;
#pragma unroll
                for (int p = 0; p < D; p++) v += Jm[r_ * gld + p] * Vm[(D + p) * gld + c];
            } else v = Jm[r_ * gld + c];
            Tb[(size_t)b * gstride + r_ * gld + c] = v;
            Tb[(size_t)b * gstride + c * gld + r_] = v;
        }
        T.sync();
        STAMP(44);  // conditional targets (pinv + products)
        int st_ = get_edges(cnt, 2, pairs);
        if (st_ != SPG_OK) { status = st_; finish_glc(); return; }
        STAMP(49);  // pair edges done
    }
    finish_glc();
    return;
}
