"""Reference of the per-blanket KLD of GLC removals (SPG_FLAG_GLC_KLD, include/spg.h). TEST HELPER, not product code.

A restatement of the definition, none of the kernel's code:

  A     = sum_e (W_e G_e)^T (W_e G_e) over the emitted GLC edges, in emission order
  G_e   = Jacobian of the edge's reparametrisation with respect to the update coordinates of its vertices: the first
          pose absolute (against the origin), the others relative to the first, each as the pose-pose error against the
          recorded measurement. Central differences at 60 digits (tests/geom_ref.py).
  N^    = orthonormal basis of the blanket's gauge: the derivative, in every kept vertex's update coordinates, of moving
          the whole blanket by one rigid motion g (X -> g X), again by central differences
  C     = Lambda_t + N^ N^^T,  r = n - d
  kld   = 1/2 ( tr(C^-1 A) - log det(A + N^ N^^T) + log det C - r )

Lambda_t is the target information the run under test reports (spg_result.target_info); W_e and the measurements are the
records of its new edges. The linear algebra runs in multiprecision as well, so the value carries no rounding of its own
beyond that of its inputs. Needs mpmath.
"""
import mpmath as mp

from tests import geom_ref as G

H = G.H_STEP


def _meas_pose(d, seg):
    """d numbers of a GLC measurement -> pose: (x, y, theta) | (t, vec(q)) with w = sqrt(1 - |vec|^2)"""
    seg = G.vec(seg)
    if d == 3:
        return seg
    w = mp.sqrt(1 - (seg[3] ** 2 + seg[4] ** 2 + seg[5] ** 2))
    return seg[:3], [seg[3], seg[4], seg[5], w]


def _origin(d):
    return G.se2([0, 0, 0]) if d == 3 else G.se3([0, 0, 0, 0, 0, 0, 1])


def reparam_jacobian(d, poses, meas):
    """dq x dq Jacobian of the reparametrisation of q poses (raw 3 | 7 numbers each) at the measurement `meas`"""
    q = len(poses)
    X = [G.pose(d, p) for p in poses]
    J = mp.zeros(d * q, d * q)
    for i in range(q):
        Z = _meas_pose(d, meas[d * i:d * (i + 1)])
        _, Ji, Jj = G.edge_terms(d, _origin(d) if i == 0 else X[0], X[i], Z)
        for r in range(d):
            for c in range(d):
                if i > 0:
                    J[d * i + r, c] = Ji[r][c]
                J[d * i + r, d * i + c] = Jj[r][c]
    return J


def _moved(d, X, g):
    """update-coordinate displacement of pose X when the world moves by g: X -> g X"""
    if d == 3:
        c, s = mp.cos(g[2]), mp.sin(g[2])
        return [c * X[0] - s * X[1] + g[0] - X[0], s * X[0] + c * X[1] + g[1] - X[1], g[2]]
    gq = [g[3], g[4], g[5], mp.sqrt(1 - (g[3] ** 2 + g[4] ** 2 + g[5] ** 2))]
    E = G.se3_mul(G.se3_inv(X), G.se3_mul((list(g[:3]), gq), X))
    q = E[1] if E[1][3] >= 0 else [-c for c in E[1]]
    return list(E[0]) + list(q[:3])


def gauge_basis(d, poses):
    """n x d orthonormal basis of the rigid motions of the whole blanket"""
    X = [G.pose(d, p) for p in poses]
    n = d * len(X)
    N = mp.zeros(n, d)
    for c in range(d):
        disp = []
        for s in (1, -1):
            g = [mp.mpf(0)] * d
            g[c] = s * H
            disp.append([v for x in X for v in _moved(d, x, g)])
        for i in range(n):
            N[i, c] = (disp[0][i] - disp[1][i]) / (2 * H)
    Q, _ = mp.qr(N, mode="skinny")
    return Q


def _logdet_spd(M):
    L = mp.cholesky(M)
    return 2 * sum(mp.log(L[i, i]) for i in range(M.rows))


def blanket_kld(d, kept_poses, lam, edges):
    """kept_poses: raw poses of the k kept vertices in target order; lam: n x n target information (array-like);
    edges: [(kept-local vertex indices, record)] with record = measurement (d q) then W (r x d q) row-major.
    Returns (kld as float, None) or (None, reason) where the value is not defined: a root edge, or edges that carry other
    than n - d rows."""
    k = len(kept_poses)
    n = d * k
    rows = 0
    for vl, rec in edges:
        if len(vl) == 1:
            return None, "root edge"
        rows += (len(rec) - d * len(vl)) // (d * len(vl))
    if rows != n - d:
        return None, f"{rows} rows for rank {n - d}"
    A = mp.zeros(n, n)
    for vl, rec in edges:
        dq = d * len(vl)
        re = (len(rec) - dq) // dq
        J = reparam_jacobian(d, [kept_poses[v] for v in vl], rec[:dq])
        W = mp.matrix(re, dq)
        for r in range(re):
            for c in range(dq):
                W[r, c] = mp.mpf(float(rec[dq + r * dq + c]))
        WG = W * J
        Ae = WG.T * WG
        idx = [d * v + c for v in vl for c in range(d)]
        for a, ia in enumerate(idx):
            for b, ib in enumerate(idx):
                A[ia, ib] += Ae[a, b]
    N = gauge_basis(d, kept_poses)
    NN = N * N.T
    Lm = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            Lm[i, j] = mp.mpf(float(lam[i][j]))
    Lm = (Lm + Lm.T) / 2
    C = Lm + NN
    Ci = mp.inverse(C)
    tr = sum(Ci[i, j] * A[j, i] for i in range(n) for j in range(n))
    return float((tr - _logdet_spd(A + NN) + _logdet_spd(C) - (n - d)) / 2), None
