"""Factor descent for NFR blankets without a closed form (SPG_FLAG_NFR_FACTOR_DESCENT, include/spg.h).
TEST HELPER, not product code: a float64 numpy restatement of the algorithm as the header states it, none of the kernel's
code. Inputs of one blanket: its target information Lambda_t (n x n over the kept vertices), the pattern as pairs of
local kept indices, and the kept vertices' poses.

  J_e     Jacobians of the new measurements by central differences of the measurement function (order 8, extended precision). The
          function only sees relative poses, so it is evaluated in the frame of the edge's first vertex: nothing of the size
          of the map coordinates enters the differences.
  U, S    spectrum of Lambda_t: the d smallest eigenvalues dropped; with more than d below 1e-5, chooseDimensions
          (src/logdet_function.cpp:40-59): of those candidates the d whose image under the new Jacobians is smallest go,
          the others stay with 1 / lambda clamped at 1e6 / lambda_max
  T_e = J~_e S J~_e^T,  M = sum_e J~_e^T X_e J~_e,  P = M^-1,  KLD = 1/2 (tr(S M) - log det M - sum log S - r)
  start   X_e = T_e^-1
  edge e  A = J~_e P J~_e^T, Psi = A^-1 - X_e, T_e = L L^T, sym(L^T Psi L) = V diag(psi) V^T,
          X_e <- L^-T V diag(max(1 - psi, 1e-9)) V^T L^-1
  P       never carried from edge to edge: every edge solves with the current M afresh (no Woodbury drift); woodbury=True instead applies
          P <- P - B^T K B, B = J~_e P, K = (I + dX A)^-1 dX within a cycle and inverts M once per cycle, as the device
          does: the difference of the two is the algorithm's own rounding sensitivity
  stop    after the first cycle whose KLD decrease is <= rel_tol max(1, |KLD|) (rel_tol = 0: never), or after max_cycles
"""
import numpy as np

FLOOR = 1e-9
ST_OK, ST_CLOSED_FORM_NOT_PD, ST_KLD_NOT_PD = 0, 5, 6


# ------------------------------------------------------------------------------------------ measurement functions
def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], _X)


def _qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]], _X)


def _qrot(q, v):
    return _qmul(_qmul(q, np.array([v[0], v[1], v[2], 0.0], _X)), _qconj(q))[:3]


def _mul(A, B):
    return A[0] + _qrot(A[1], B[0]), _qmul(A[1], B[1])


def _inv(A):
    qi = _qconj(A[1])
    return -_qrot(qi, A[0]), qi


def _se3(p):
    p = np.asarray(p, _X)
    return p[:3].copy(), p[3:7] / np.sqrt(p[3:7] @ p[3:7])


def _se3_error(rel, z_inv, da, db):
    """[t, vec q] of Z^-1 (Xa [+] da)^-1 (Xb [+] db) with rel = Xa^-1 Xb; X [+] d = X * (d[:3], (d[3:], sqrt(1 - |d[3:]|^2)))"""
    inc = lambda dd: (dd[:3], np.array([dd[3], dd[4], dd[5], np.sqrt(1 - dd[3:] @ dd[3:])], _X))
    E = _mul(z_inv, _mul(_inv(inc(da)), _mul(rel, inc(db))))
    q = E[1] / np.sqrt(E[1] @ E[1])
    if q[3] < 0:
        q = -q
    return np.concatenate([E[0], q[:3]])


def _se2_error(rel, da, db):
    """EdgeSE2 with additive updates, z = the measurement at the linearisation point; rel = (R_a^T (t_b - t_a), th_b - th_a, th_a)"""
    dt, dth, tha = rel
    # R(th_a + da_th)^T (t_b + db_t - t_a - da_t) = R(da_th)^T (dt + R(th_a)^T (db_t - da_t))
    c0, s0 = np.cos(tha), np.sin(tha)
    w = db[:2] - da[:2]
    v = dt + np.array([c0 * w[0] + s0 * w[1], -s0 * w[0] + c0 * w[1]], _X)
    c, s = np.cos(da[2]), np.sin(da[2])
    return np.array([c * v[0] + s * v[1] - dt[0], -s * v[0] + c * v[1] - dt[1], db[2] - da[2]], _X)


# Central differences of order 8: weights of f(x + i h) - f(x - i h), i = 1 .. 4, the function evaluated in extended
# precision (np.longdouble) and the quotient rounded to float64. With h = 5e-3 the truncation error is ~ h^8 = 4e-19 of the
# function's scale (its Taylor series in an increment has a radius of convergence of order one) and the rounding error
# ~ 1e-19 / h = 2e-17 of it. The plain two-point formula in float64 cannot have both below 1e-10, and the informations of a
# hub blanket move by ten times the error of the Jacobians.
_STENCIL = (4.0 / 5.0, -1.0 / 5.0, 4.0 / 105.0, -1.0 / 280.0)
_X = np.longdouble


def jacobians(d, poses, pairs, h=5e-3, stencil=_STENCIL):
    """J_e (d x n) of every new measurement at the poses, n = d * len(poses): central differences of the measurement function."""
    poses = np.asarray(poses, _X)
    stencil = [_X(int(round(w * 840))) / _X(840) for w in stencil]
    h = _X(h)
    n = d * len(poses)
    out = []
    for a, b in pairs:
        if d == 3:
            pa, pb = poses[a], poses[b]
            c, s = np.cos(pa[2]), np.sin(pa[2])
            dx = pb[:2] - pa[:2]
            rel = (np.array([c * dx[0] + s * dx[1], -s * dx[0] + c * dx[1]], _X), pb[2] - pa[2], pa[2])
            f = lambda da, db: _se2_error(rel, da, db)
        else:
            rel = _mul(_inv(_se3(poses[a])), _se3(poses[b]))
            z_inv = _inv(rel)
            f = lambda da, db: _se3_error(rel, z_inv, da, db)
        J = np.zeros((d, n))
        for col in range(2 * d):
            def at(step):
                v = np.zeros(d, _X)
                v[col % d] = step
                return f(v, np.zeros(d, _X)) if col < d else f(np.zeros(d, _X), v)
            J[:, (a if col < d else b) * d + col % d] = (sum(w * (at((i + 1) * h) - at(-(i + 1) * h)) for i, w in enumerate(stencil)) / h).astype(float)
        out.append(J)
    return out


def spectrum(d, lam, Js):
    """(U, S, rank_deficient) of the target"""
    lam = np.asarray(lam, float)
    n = lam.shape[0]
    w, V = np.linalg.eigh(0.5 * (lam + lam.T))
    small = int((w < 1e-5).sum())
    if small <= d:
        return V[:, d:], 1.0 / w[d:], False
    Jall = np.vstack(Js)
    norms = np.array([np.linalg.norm(Jall @ V[:, c]) for c in range(small)])
    drop = sorted(np.lexsort((np.arange(small), norms))[:d].tolist())
    keep = [i for i in range(n) if i not in drop]
    return V[:, keep], np.minimum(np.abs(1.0 / w[keep]), 1e6 / w[-1]), True


def kld_of(Jt, S, X):
    """KLD of the informations X (E x d x d) or None when M is not positive definite; also M"""
    E, d, r = Jt.shape
    M = Jt.reshape(E * d, r).T @ (X @ Jt).reshape(E * d, r)
    M = 0.5 * (M + M.T)
    try:
        Lc = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return None, M
    return 0.5 * (float(np.diag(M) @ S) - 2.0 * np.log(np.diag(Lc)).sum() - np.log(S).sum() - r), M


def run(d, lam, pairs, poses, max_cycles=2000, rel_tol=1e-12, woodbury=False, Js=None):
    """-> dict(status, X (E x d x d), kld (final), trace (KLD at the start and after every cycle), cycles, hit_max, rank_deficient)"""
    Js = jacobians(d, poses, pairs) if Js is None else Js
    U, S, deficient = spectrum(d, lam, Js)
    Jt = np.stack([J @ U for J in Js])
    E, r = len(pairs), U.shape[1]
    T = np.einsum("eac,c,ebc->eab", Jt, S, Jt)
    T = 0.5 * (T + T.transpose(0, 2, 1))
    try:
        Ls = np.linalg.cholesky(T)
    except np.linalg.LinAlgError:
        return {"status": ST_CLOSED_FORM_NOT_PD, "X": np.zeros((0, d, d)), "kld": np.nan, "trace": [], "cycles": 0, "hit_max": False,
                "rank_deficient": deficient}
    Li = np.linalg.inv(Ls)
    X = Li.transpose(0, 2, 1) @ Li
    kld, M = kld_of(Jt, S, X)
    res = {"status": ST_OK, "rank_deficient": deficient, "hit_max": False}
    trace, cycles = [kld], 0
    bad = kld is None
    while not bad and cycles < max_cycles:
        P = np.linalg.inv(M)
        Xprev = X.copy()
        for e in range(E):
            # (from scratch: J~_e M^-1 J~_e^T by a fresh solve with the current M, which is all of P an edge needs)
            A = Jt[e] @ (P @ Jt[e].T if woodbury else np.linalg.solve(M, Jt[e].T))
            A = 0.5 * (A + A.T)
            Psi = np.linalg.inv(A) - X[e]
            Pt = Ls[e].T @ Psi @ Ls[e]
            psi, V = np.linalg.eigh(0.5 * (Pt + Pt.T))
            G = V.T @ Li[e]
            Xn = G.T @ (np.maximum(1.0 - psi, FLOOR)[:, None] * G)
            Xn = 0.5 * (Xn + Xn.T)
            dX = Xn - X[e]
            X[e] = Xn
            if woodbury:
                B = Jt[e] @ P
                K = np.linalg.solve(np.eye(d) + dX @ A, dX)
                P = P - B.T @ (0.5 * (K + K.T)) @ B
            else:
                M = M + Jt[e].T @ dX @ Jt[e]
                M = 0.5 * (M + M.T)
        new, M = kld_of(Jt, S, X)
        if new is None or not np.isfinite(new):
            X, bad = Xprev, True
            break
        cycles += 1
        trace.append(new)
        dec = kld - new
        kld = new
        if rel_tol > 0 and dec <= rel_tol * max(1.0, abs(new)):
            break
    else:
        res["hit_max"] = not bad
    if bad:
        res["status"], kld = ST_KLD_NOT_PD, np.nan
    res.update(X=X, kld=kld, trace=trace, cycles=cycles)
    return res
