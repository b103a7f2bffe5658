// csrc/spg_nfr_fd.inc — factor descent for the NFR patterns without a closed form (SPG_FLAG_NFR_FACTOR_DESCENT,
// DESIGN.md 5h-F): cyclic block-coordinate descent over the edge informations (Vallve, Sola, Andrade-Cetto, RA-L 2018),
// iterative proportional fitting in measurement space. A body fragment of nfr_ip_kernel<D, false, true>, included right
// after JU is filled: it replaces the barrier loop of the interior point; everything before it (gather, Schur complement,
// pattern, spectrum, JU) and the hand-over (records, out record, final word) are the kernel's own.
//
//   T_e = J~_e S J~_e^T (constant),  M(X) = sum_e J~_e^T X_e J~_e,  P = M^-1,
//   KLD(X) = 1/2 (tr(S M) - log det M - log det S - r)                                  (value() without the barrier)
//   start  X_e = T_e^-1
//   edge e A = J~_e P J~_e^T,  Psi = A^-1 - X_e,  T_e = L L^T,  sym(L^T Psi L) = V diag(psi) V^T,
//          X_e <- L^-T V diag(max(1 - psi, 1e-9)) V^T L^-1            (the exact minimiser over X_e >= 1e-9 T_e^-1)
//          P <- P - B^T K B,  B = J~_e P,  K = (I + dX A)^-1 dX        (Woodbury, rank <= d; dX may be singular)
//   cycle  all edges in pattern order, then M from X, its Cholesky (log det M, the KLD) and P = M^-1 afresh: rounding
//          drift of the rank-d updates is bounded by one cycle
//   stop   after the first cycle whose KLD decrease is <= rel_tol max(1, |KLD|), or after max_cycles
//
// Buffers (ip_layout with fd): X, its copy of the last completed cycle, L_e and L_e^-1 in the x / xn / g / gn blocks,
// W = blockdiag(X) J~ in dv, B and K B in P; M, its factor, L^-1 and P = M^-1 in M / Mc / Li / Mi. All of it is in LDS
// when it fits (`hot`); from n >= 96 the per-cycle factorisation and inverse run blocked on the matrix cores.
// The d x d step of an edge is done by wavefront 0 on small LDS matrices (the Newton solve's vector is idle here): lane
// (i, j) owns an entry, the two small inverses are done by lane 0 in registers, the spectrum by jacobi_eigh as a
// single-wavefront team. Every sum has a fixed order: two runs are bit-identical.
{
    double *const Pm = Mi;
    double *const Xf = hot + L.x, *const Xbak = hot + L.xn, *const Lt = hot + L.g, *const Lti = hot + L.gn;
    double *const Wm = hot + L.dv, *const Bb = hot + L.P, *const Cb = Bb + D * r;
    double *const sA = colbuf, *const sAi = colbuf + 40, *const sPsi = colbuf + 80, *const sPt = colbuf + 120, *const sV = colbuf + 160,
                 *const sG = colbuf + 200, *const sDX = colbuf + 240, *const sF = colbuf + 280, *const sK = colbuf + 320, *const scs = colbuf + 360;
    const bool fd_big = n >= 96 && hot == ws + L.cold_total && kBlockedLds <= a.lds_doubles;
    constexpr double kFloor = 1e-9;

    // ---- T_e (lower triangle) into the L_e blocks
    for (int it = tid; it < E * DD; it += NT) {
        const int e = it / DD, i = (it - e * DD) / D, j = it - e * DD - i * D;
        if (j <= i) {
            const double *Ji = JU + (int64_t)(e * D + i) * r, *Jj = JU + (int64_t)(e * D + j) * r;
            double s = 0;
            for (int c = 0; c < r; c++) s += Ji[c] * Sv[c] * Jj[c];
            Lt[it] = s;
        }
    }
    if (tid == 0) flag_s = 0;
    __syncthreads();
    // ---- T_e = L L^T, L^-1, start X_e = L^-T L^-1 (one lane per edge, registers)
    for (int e = tid; e < E; e += NT) {
        double B[DD], rB[D], Iv[DD];
#pragma unroll
        for (int i = 0; i < D; i++)
#pragma unroll
            for (int j = 0; j < D; j++) B[i * D + j] = (j <= i) ? Lt[e * DD + i * D + j] : 0.0;
        if (!chol_static<D>(B, rB)) { flag_s = 1; continue; }
#pragma unroll
        for (int c = 0; c < D; c++)
#pragma unroll
            for (int i = 0; i < D; i++) {
                if (i < c) Iv[i * D + c] = 0.0;
                else {
                    double s = (i == c) ? 1.0 : 0.0;
#pragma unroll
                    for (int t = c; t < i; t++) s -= B[i * D + t] * Iv[t * D + c];
                    Iv[i * D + c] = div_by(s, B[i * D + i], rB[i]);
                }
            }
#pragma unroll
        for (int i = 0; i < D; i++)
#pragma unroll
            for (int j = 0; j < D; j++) {
                Lt[e * DD + i * D + j] = (j <= i) ? B[i * D + j] : 0.0;
                Lti[e * DD + i * D + j] = Iv[i * D + j];
                const int lo = i < j ? i : j, hi = i < j ? j : i;
                double s = 0;
#pragma unroll
                for (int t = 0; t < D; t++) if (t >= hi) s += Iv[t * D + hi] * Iv[t * D + lo];
                Xf[e * DD + i * D + j] = s;
            }
    }
    __syncthreads();
    if (flag_s) { status = SPG_ST_CLOSED_FORM_NOT_PD; n_new = 0; finish(); return; }

    // ---- M from X, its Cholesky, the KLD, P = M^-1; false when M is not positive definite
    auto fd_eval = [&](double &val) -> bool {
        for (int it = tid; it < q * r; it += NT) {
            const int row = it / r, c = it - row * r, e = row / D, p = row - e * D;
            const double *Xe = Xf + e * DD + p * D, *Je = JU + (int64_t)e * D * r + c;
            double s = 0;
#pragma unroll
            for (int t = 0; t < D; t++) s += Xe[t] * Je[(int64_t)t * r];
            Wm[it] = s;
        }
        __syncthreads();
        if (fd_big) team_gemm<NT>(T, M, r, JU, r, true, Wm, r, false, r, r, q, 0, true, lds_pool);      // lower block triangle
        else {
            for (int it = tid; it < r * r; it += NT) {
                const int i = it / r, j = it - i * r;
                if (j <= i) {
                    double s = 0;
#pragma unroll 4
                    for (int t = 0; t < q; t++) s += JU[(int64_t)t * r + i] * Wm[(int64_t)t * r + j];
                    M[it] = s;
                }
            }
            __syncthreads();
        }
        for (int it = tid; it < r * r; it += NT) { const int i = it / r, j = it - i * r; if (j > i) M[it] = M[j * r + i]; }
        __syncthreads();
        double tr = 0;
        for (int i = tid; i < r; i += NT) tr += M[i * r + i] * Sv[i];
        tr = T.sum(tr);
        for (int it = tid; it < r * r; it += NT) Mc[it] = M[it];
        if (tid == 0) flag_s = 0;
        __syncthreads();
        if (fd_big) chol_lower_blocked<NT>(T, Mc, r, r, T1, lds_pool);
        else chol_lower<NT>(T, Mc, r, r);
        __syncthreads();
        const bool okc = flag_s == 0;
        __syncthreads();
        if (!okc) { if (tid == 0) flag_s = 0; __syncthreads(); return false; }
        double l = 0;
        for (int i = tid; i < r; i += NT) l += log(Mc[i * r + i]);
        l = T.sum(l);
        val = 0.5 * (tr - 2.0 * l - logdetS - r);
        if (fd_big) {
            tri_inverse_lower_blocked<NT>(T, Mc, r, Li, r, r, T1, lds_pool);
            team_gemm<NT>(T, Pm, r, Li, r, true, Li, r, false, r, r, r, 0, true, lds_pool);
            for (int it = tid; it < r * r; it += NT) { const int i = it / r, j = it - i * r; if (j > i) Pm[it] = Pm[j * r + i]; }
            __syncthreads();
        } else {
            tri_inverse_lower<NT>(T, Mc, Li, r, r);
            gram_lower_inverse<NT>(T, Li, Pm, r, r);
        }
        return true;
    };

    // ---- the d x d step of edge e by wavefront 0: sA = A in, X_e updated, sK = K out; si[0] != 0 on failure
    auto fd_edge_step = [&](int e) {
        double *Xe = Xf + e * DD;
        const double *Le = Lt + e * DD, *Lie = Lti + e * DD;
        const Team<64> W{tid, red, &flag_s};
        const int lane = tid, i = lane / D, j = lane - (lane / D) * D;
        const bool ent = lane < DD, low = ent && j <= i;
        if (lane == 0) {     // A^-1
            double B[DD], rB[D], Iv[DD];
#pragma unroll
            for (int t = 0; t < DD; t++) B[t] = sA[t];
            if (!chol_static<D>(B, rB)) si[0] = 1;
            else {
#pragma unroll
                for (int c = 0; c < D; c++) {
                    double y[D];
#pragma unroll
                    for (int u = 0; u < D; u++) {
                        double s = (u == c) ? 1.0 : 0.0;
#pragma unroll
                        for (int t = 0; t < u; t++) s -= B[u * D + t] * y[t];
                        y[u] = div_by(s, B[u * D + u], rB[u]);
                    }
#pragma unroll
                    for (int u = D - 1; u >= 0; u--) {
                        double s = y[u];
#pragma unroll
                        for (int t = u + 1; t < D; t++) s -= B[t * D + u] * Iv[t * D + c];
                        Iv[u * D + c] = div_by(s, B[u * D + u], rB[u]);
                    }
                }
#pragma unroll
                for (int t = 0; t < DD; t++) sAi[t] = Iv[t];
            }
        }
        W.sync();
        if (si[0]) return;
        if (low) { const double v = 0.5 * (sAi[i * D + j] + sAi[j * D + i]) - Xe[i * D + j]; sPsi[i * D + j] = v; sPsi[j * D + i] = v; }      // Psi
        W.sync();
        if (ent) { double s = 0; for (int t = 0; t < D; t++) s += sPsi[i * D + t] * Le[t * D + j]; sG[lane] = s; }                          // Psi L
        W.sync();
        if (low) {                                                                                                                           // sym(L^T Psi L)
            double s1 = 0, s2 = 0;
            for (int t = 0; t < D; t++) { s1 += Le[t * D + i] * sG[t * D + j]; s2 += Le[t * D + j] * sG[t * D + i]; }
            const double v = 0.5 * (s1 + s2);
            sPt[i * D + j] = v; sPt[j * D + i] = v;
        }
        W.sync();
        if (!jacobi_eigh<64>(W, sPt, sV, D, D, scs)) { if (lane == 0) si[0] = 2; W.sync(); return; }
        if (ent) { double s = 0; for (int t = 0; t < D; t++) s += sV[t * D + i] * Lie[t * D + j]; sG[lane] = s; }                           // G = V^T L^-1
        W.sync();
        if (low) {                                                                                                                           // X_e, dX
            double s = 0;
            for (int t = 0; t < D; t++) s += (fmax(1.0 - sPt[t * D + t], kFloor) * sG[t * D + i]) * sG[t * D + j];
            const double dx = s - Xe[i * D + j];
            Xe[i * D + j] = s; Xe[j * D + i] = s;
            sDX[i * D + j] = dx; sDX[j * D + i] = dx;
        }
        W.sync();
        if (ent) { double s = (i == j) ? 1.0 : 0.0; for (int t = 0; t < D; t++) s += sDX[i * D + t] * sA[t * D + j]; sF[lane] = s; }       // I + dX A
        W.sync();
        if (lane == 0) {
            double F[DD], Fi[DD];
#pragma unroll
            for (int t = 0; t < DD; t++) F[t] = sF[t];
            if (!small_inverse<D>(F, Fi)) si[0] = 3;
#pragma unroll
            for (int t = 0; t < DD; t++) sF[t] = Fi[t];
        }
        W.sync();
        if (si[0]) return;
        if (ent) { double s = 0; for (int t = 0; t < D; t++) s += sF[i * D + t] * sDX[t * D + j]; sG[lane] = s; }                            // (I + dX A)^-1 dX
        W.sync();
        if (low) { const double v = 0.5 * (sG[i * D + j] + sG[j * D + i]); sK[i * D + j] = v; sK[j * D + i] = v; }
        W.sync();
    };

    const int max_cycles = a.fd_max_cycles;
    const double rel_tol = a.fd_rel_tol;
    double kld_cur = 0;
    bool fd_fail = !fd_eval(kld_cur) || !isfinite(kld_cur), fd_restore = false, fd_converged = false;
    int cycles = 0;
    while (!fd_fail && cycles < max_cycles) {
        for (int it = tid; it < nx; it += NT) Xbak[it] = Xf[it];
        if (tid == 0) si[0] = 0;
        __syncthreads();
        fd_restore = true;
        for (int e = 0; e < E; e++) {
            const double *Je = JU + (int64_t)e * D * r;
            for (int it = tid; it < D * r; it += NT) {                     // B = J~_e P
                const int p = it / r, c = it - p * r;
                double s = 0;
#pragma unroll 4
                for (int t = 0; t < r; t++) s += Je[p * r + t] * Pm[t * r + c];
                Bb[it] = s;
            }
            __syncthreads();
            if (tid < DD) {                                                // A = B J~_e^T
                const int i = tid / D, j = tid - i * D;
                if (j <= i) {
                    double s = 0;
                    for (int c = 0; c < r; c++) s += Bb[i * r + c] * Je[j * r + c];
                    sA[i * D + j] = s; sA[j * D + i] = s;
                }
            }
            __syncthreads();
            if (tid < 64) fd_edge_step(e);
            __syncthreads();
            if (si[0]) break;
            for (int it = tid; it < D * r; it += NT) {                     // K B
                const int p = it / r, c = it - p * r;
                double s = 0;
#pragma unroll
                for (int t = 0; t < D; t++) s += sK[p * D + t] * Bb[t * r + c];
                Cb[it] = s;
            }
            __syncthreads();
            for (int it = tid; it < r * r; it += NT) {                     // P -= B^T (K B)
                const int i = it / r, j = it - i * r;
                if (j <= i) {
                    double s = 0;
#pragma unroll
                    for (int t = 0; t < D; t++) s += Bb[t * r + i] * Cb[t * r + j];
                    const double v = Pm[it] - s;
                    Pm[it] = v; Pm[j * r + i] = v;
                }
            }
            __syncthreads();
        }
        if (si[0]) { fd_fail = true; break; }
        double kld_new = 0;
        if (!fd_eval(kld_new) || !isfinite(kld_new)) { fd_fail = true; break; }
        cycles++;
        const double dec = kld_cur - kld_new;
        kld_cur = kld_new;
        if (rel_tol > 0 && dec <= rel_tol * fmax(1.0, fabs(kld_new))) { fd_converged = true; break; }
    }
    if (fd_fail) {
        // the model of the running cycle is not positive definite: the edges of the last completed cycle, no KLD
        if (fd_restore) { for (int it = tid; it < nx; it += NT) Xf[it] = Xbak[it]; }
        status = SPG_ST_KLD_NOT_PD;
        __syncthreads();
    } else {
        kld = kld_cur;
        if (!fd_converged) info |= SPG_INFO_FD_MAX_CYCLES;
    }
    info |= min(cycles, 32767) << 8;
    // information of the new edges: upper triangle, row by row
    for (int it = tid; it < E * (D * (D + 1) / 2); it += NT) {
        const int e = it / (D * (D + 1) / 2);
        int o = it - e * (D * (D + 1) / 2), i = 0;
        while (o >= D - i) { o -= D - i; i++; }
        const int j = i + o;
        arena[bd.new_off + (int64_t)e * REC + PS + (it - e * (D * (D + 1) / 2))] = Xf[e * DD + i * D + j];
    }
    n_new = E;
    finish();
    return;
}
