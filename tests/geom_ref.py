"""Independent multiprecision reference of the SE2 / SE3 pose-pose edge geometry (TEST HELPER, not product code).

Everything is derived from the definitions, not from the kernel's formulas (csrc/spg_dev_geom.hpp, oracle/ref_geom.hpp):

  SE3 pose   X = (t, q) with q = (x, y, z, w) a unit quaternion (stored values are normalised on entry)
  product    A * B = (t_A + q_A t_B q_A^-1, q_A (x) q_B)         Hamilton product, rotations applied as q v q^-1
  error      e(Xi, Xj, Z) = [t_E, vec(q_E)],  E = Z^-1 Xi^-1 Xj,  q_E = q_Z^-1 (x) q_i^-1 (x) q_j normalised, w >= 0
  update     X [+] d = X * (d[:3], (d[3:], sqrt(1 - |d[3:]|^2)))
  Jacobians  central differences of e under [+] with h = 1e-20 at 60 digits (truncation ~ h^2 = 1e-40)

There is no rotation matrix anywhere, so none of the branches of R_to_quat / dq_dR exists here. Two conventions are needed to
make the differences well defined where e itself jumps:
  * the perturbed q_E takes the sign that is closest to the unperturbed one (the error lives on the sphere of unit
    quaternions; its w >= 0 chart jumps at w == 0, the derivative does not),
  * the angle of an SE2 error is differenced on the circle (wrapped before it is divided by 2h).

SE2 follows EdgeSE2ISAM: pose (x, y, theta), additive update, error [R(theta_i)^T (t_j - t_i) - z_t,
normalize(normalize(theta_j - theta_i) - z_theta)]. normalize_theta is g2o's, whose pi is the fp64 constant M_PI: that
constant, not the real number, defines the interval [-pi, pi) and the period here too.

Needs mpmath; the GPU tests read tests/golden/geometry_cases.npz (tests/golden/make_geometry_cases.py) instead.
"""
import math

import mpmath as mp

mp.mp.dps = 60
H_STEP = mp.mpf(10) ** -20
PI64 = mp.mpf(math.pi)


def vec(x):
    """float64 values -> exact multiprecision numbers"""
    return [x_ if isinstance(x_, mp.mpf) else mp.mpf(float(x_)) for x_ in x]


# ------------------------------------------------------------------------------------------ quaternions (x, y, z, w)
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw,
            aw * bw - ax * bx - ay * by - az * bz]


def qconj(q):
    return [-q[0], -q[1], -q[2], q[3]]


def qunit(q):
    n = mp.sqrt(sum(c * c for c in q))
    return [c / n for c in q]


def qrot(q, v):
    """q v q^-1 for a unit q"""
    return qmul(qmul(q, [v[0], v[1], v[2], mp.mpf(0)]), qconj(q))[:3]


def axis_angle(axis, deg):
    a = vec(axis)
    n = mp.sqrt(sum(c * c for c in a))
    half = mp.mpf(deg) * mp.pi / 360
    s = mp.sin(half)
    return [a[0] / n * s, a[1] / n * s, a[2] / n * s, mp.cos(half)]


# ------------------------------------------------------------------------------------------ SE3
def se3(p):
    """7 stored numbers -> (t, unit q)"""
    p = vec(p)
    return p[:3], qunit(p[3:7])


def se3_mul(A, B):
    r = qrot(A[1], B[0])
    return [A[0][i] + r[i] for i in range(3)], qmul(A[1], B[1])


def se3_inv(A):
    qi = qconj(A[1])
    r = qrot(qi, A[0])
    return [-r[0], -r[1], -r[2]], qi


def _canonical(q, toward=None):
    q = qunit(q)
    if toward is None:
        flip = q[3] < 0
    else:
        flip = sum(a * b for a, b in zip(q, toward)) < 0
    return [-c for c in q] if flip else q


def se3_error_full(Xi, Xj, Z, toward=None):
    E = se3_mul(se3_inv(Z), se3_mul(se3_inv(Xi), Xj))
    return E[0], _canonical(E[1], toward)


def se3_error(Xi, Xj, Z):
    t, q = se3_error_full(Xi, Xj, Z)
    return t + q[:3]


def se3_oplus(X, d):
    w = mp.sqrt(1 - (d[3] * d[3] + d[4] * d[4] + d[5] * d[5]))
    return se3_mul(X, (list(d[:3]), [d[3], d[4], d[5], w]))


def se3_between(Xi, Xj):
    """measurement from state: Xi^-1 Xj as 7 numbers, unit quaternion with w >= 0"""
    B = se3_mul(se3_inv(Xi), Xj)
    return B[0] + _canonical(B[1])


def se3_jacobians(Xi, Xj, Z):
    """(err[6], Ji[6][6], Jj[6][6]) of e(Xi [+] di, Xj [+] dj, Z) at 0"""
    t0, q0 = se3_error_full(Xi, Xj, Z)
    Ji = [[None] * 6 for _ in range(6)]
    Jj = [[None] * 6 for _ in range(6)]
    for c in range(6):
        for J, which in ((Ji, 0), (Jj, 1)):
            e = []
            for s in (1, -1):
                d = [mp.mpf(0)] * 6
                d[c] = s * H_STEP
                a = se3_oplus(Xi, d) if which == 0 else Xi
                b = se3_oplus(Xj, d) if which == 1 else Xj
                t, q = se3_error_full(a, b, Z, toward=q0)
                e.append(t + q[:3])
            for r in range(6):
                J[r][c] = (e[0][r] - e[1][r]) / (2 * H_STEP)
    return t0 + q0[:3], Ji, Jj


def se3_diff(Xb, Xo):
    """estimateDifference (src/graph_wrapper_g2o.cpp:550-575): compact vector of Xb^-1 Xo"""
    B = se3_mul(se3_inv(Xb), Xo)
    return B[0] + _canonical(B[1])[:3]


# ------------------------------------------------------------------------------------------ SE2
def normalize_theta(th):
    if -PI64 <= th < PI64:
        return th
    m = th - mp.floor(abs(th) / (2 * PI64)) * (2 * PI64) * mp.sign(th)    # fmod: the sign of th, magnitude below 2 pi
    if m >= PI64:
        m -= 2 * PI64
    if m < -PI64:
        m += 2 * PI64
    return m


def se2(p):
    return vec(p)


def se2_between(xi, xj):
    c, s = mp.cos(xi[2]), mp.sin(xi[2])
    dx, dy = xj[0] - xi[0], xj[1] - xi[1]
    return [c * dx + s * dy, -s * dx + c * dy, normalize_theta(xj[2] - xi[2])]


def se2_error(xi, xj, z):
    d = se2_between(xi, xj)
    return [d[0] - z[0], d[1] - z[1], normalize_theta(d[2] - z[2])]


def se2_jacobians(xi, xj, z):
    e0 = se2_error(xi, xj, z)
    Ji = [[None] * 3 for _ in range(3)]
    Jj = [[None] * 3 for _ in range(3)]
    for c in range(3):
        for J, which in ((Ji, 0), (Jj, 1)):
            e = []
            for s in (1, -1):
                a, b = list(xi), list(xj)
                (a if which == 0 else b)[c] += s * H_STEP
                e.append(se2_error(a, b, z))
            for r in range(3):
                dlt = e[0][r] - e[1][r]
                J[r][c] = (normalize_theta(dlt) if r == 2 else dlt) / (2 * H_STEP)
    return e0, Ji, Jj


def se2_diff(xb, xo):
    return [xb[0] - xo[0], xb[1] - xo[1], normalize_theta(xb[2] - xo[2])]


# ------------------------------------------------------------------------------------------ graphs
def pose(d, p):
    return se3(p) if d == 6 else se2(p)


def edge_terms(d, Xi, Xj, Z):
    return se3_jacobians(Xi, Xj, Z) if d == 6 else se2_jacobians(Xi, Xj, Z)


def between(d, Xi, Xj):
    return se3_between(Xi, Xj) if d == 6 else se2_between(Xi, Xj)


def diff(d, Xb, Xo):
    return se3_diff(Xb, Xo) if d == 6 else se2_diff(Xb, Xo)


def omega(d, upper):
    """row-wise upper triangle (the edge record of include/spg.h) -> full symmetric matrix"""
    u = vec(upper)
    om = [[None] * d for _ in range(d)]
    p = 0
    for i in range(d):
        for j in range(i, d):
            om[i][j] = om[j][i] = u[p]
            p += 1
    return om


def chi2_and_information(d, poses, edges, with_H=True):
    """poses: {id: pose}, edges: [(i, j, Z, Omega full)]. Returns (chi2, H over ALL vertices in id order as nested lists):
    chi2 = sum e^T Omega e, H = sum J^T Omega J; the caller drops the fixed vertex's rows and columns."""
    ids = sorted(poses)
    loc = {v: k for k, v in enumerate(ids)}
    n = d * len(ids)
    H = [[mp.mpf(0)] * n for _ in range(n)] if with_H else None
    chi2 = mp.mpf(0)
    for i, j, Z, om in edges:
        if with_H:
            e, Ji, Jj = edge_terms(d, poses[i], poses[j], Z)
        else:
            e = se3_error(poses[i], poses[j], Z) if d == 6 else se2_error(poses[i], poses[j], Z)
        chi2 += sum(e[a] * om[a][b] * e[b] for a in range(d) for b in range(d))
        if not with_H:
            continue
        blocks = ((loc[i], Ji), (loc[j], Jj))
        for va, Ja in blocks:
            OJ = [[sum(om[r][k] * Ja[k][c] for k in range(d)) for c in range(d)] for r in range(d)]   # Omega Ja
            for vb, Jb in blocks:
                for r in range(d):
                    for c in range(d):
                        H[vb * d + r][va * d + c] += sum(Jb[k][r] * OJ[k][c] for k in range(d))
    return chi2, H


def to_float(x):
    if isinstance(x, (list, tuple)):
        return [to_float(v) for v in x]
    return float(x)
