"""Plain numpy reference of the relative-pose covariance and the candidate-edge scores (TEST HELPER, not product code):
spg_graph_relative_covariances / spg_graph_score_candidates, include/spg.h.

Conventions (those of spg_graph_information): an SE2 pose is (x, y, theta) with the additive update, an SE3 pose is
(t, unit quaternion x y z w) with the update X <- X * fromVectorMQT(delta); the error of a binary edge a -> b with
measurement z is e = between(xa, xb) - z (angle wrapped twice) for SE2 and toVectorMQT(Z^-1 Xa^-1 Xb) for SE3, and
J = [Ja Jb] are its analytic Jacobians with respect to the two updates. With Sigma_ab the 2D x 2D joint covariance of the
pair and Omega the information of the candidate:

    P    = J Sigma_ab J^T
    chi2 = e^T Omega e
    d2   = e^T (P + Omega^-1)^-1 e          np.linalg.solve(P + inv(Omega), e)
    gain = 1/2 ln det(I + Omega P)          np.linalg.slogdet

d2 and gain deliberately do not take the device's route (Omega = L L^T, M = I + L^T P L): the inverse of Omega is formed
here and never there. Numpy only: the GPU tests import this module.
"""
import numpy as np

PI = 3.14159265358979323846


# ------------------------------------------------------------------------------------------ SE2
def normalize_theta(th):
    if -PI <= th < PI:
        return th
    m = np.fmod(th, 2.0 * PI)
    if m >= PI:
        m -= 2.0 * PI
    if m < -PI:
        m += 2.0 * PI
    return m


def se2_between(xi, xj):
    c, s = np.cos(xi[2]), np.sin(xi[2])
    dx, dy = xj[0] - xi[0], xj[1] - xi[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, normalize_theta(xj[2] - xi[2])])


def se2_edge(xi, xj, z):
    """(err[3], Ji[3, 3], Jj[3, 3])"""
    c, s = np.cos(xi[2]), np.sin(xi[2])
    dx, dy = xj[0] - xi[0], xj[1] - xi[1]
    err = np.array([c * dx + s * dy - z[0], -s * dx + c * dy - z[1], normalize_theta(normalize_theta(xj[2] - xi[2]) - z[2])])
    Ji = np.array([[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy], [0.0, 0.0, -1.0]])
    Jj = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    return err, Ji, Jj


# ------------------------------------------------------------------------------------------ SE3
def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_to_quat(R):
    """unit quaternion (x, y, z, w) with w >= 0 (Shepperd's four branches)"""
    q = np.zeros(4)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        r = np.sqrt(t + 1.0)
        q[3] = 0.5 * r
        r = 0.5 / r
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * r, (R[0, 2] - R[2, 0]) * r, (R[1, 0] - R[0, 1]) * r
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        r = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * r
        r = 0.5 / r
        q[3] = (R[k, j] - R[j, k]) * r
        q[j] = (R[j, i] + R[i, j]) * r
        q[k] = (R[k, i] + R[i, k]) * r
    q /= np.linalg.norm(q)
    return -q if q[3] < 0 else q


def iso(p):
    """7 stored numbers -> (R, t); the stored quaternion is used as given"""
    p = np.asarray(p, np.float64)
    return quat_to_R(p[3:7]), p[:3].copy()


def iso_inv_mul(A, B):
    """A^-1 B"""
    return A[0].T @ B[0], A[0].T @ (B[1] - A[1])


def se3_between(xi, xj):
    R, t = iso_inv_mul(iso(xi), iso(xj))
    return np.concatenate([t, R_to_quat(R)])


def _dq_dR(R):
    """D[comp, row, col] = d(compact quaternion)[comp] / dR[row, col], the sign of the w >= 0 chart"""
    D = np.zeros((3, 3, 3))
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        S = np.sqrt(tr + 1.0) * 2
        qw = 0.25 * S
        n = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        g = -2.0 / (S * S * S)
        for a in range(3):
            D[:, a, a] = n * g
        D[0, 2, 1], D[0, 1, 2] = 1 / S, -1 / S
        D[1, 0, 2], D[1, 2, 0] = 1 / S, -1 / S
        D[2, 1, 0], D[2, 0, 1] = 1 / S, -1 / S
    else:
        if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
            i = 0
        elif R[1, 1] > R[2, 2]:
            i = 1
        else:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        S = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        qw = (R[k, j] - R[j, k]) / S
        nj, nk = R[i, j] + R[j, i], R[i, k] + R[k, i]
        for a in range(3):
            dS = (2.0 if a == i else -2.0) / S
            D[i, a, a] = 0.25 * dS
            D[j, a, a] = -nj / (S * S) * dS
            D[k, a, a] = -nk / (S * S) * dS
        D[j, i, j] = D[j, j, i] = 1 / S
        D[k, i, k] = D[k, k, i] = 1 / S
    return -D if qw <= 0 else D


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def se3_edge(xi, xj, z):
    """(err[6], Ji[6, 6], Jj[6, 6]) of err = toVectorMQT(Z^-1 Xi^-1 Xj) under X <- X * fromVectorMQT(delta): with
    B = Xi^-1 Xj and E = Z^-1 B, a translation step of Xj moves t_E by R_E, one of Xi by -R_Z^T; a rotation step with compact
    quaternion dq turns the frame by I + 2 [dq]x, which moves t_E by R_Z^T 2 [t_B]x (Xi) and R_E by -R_Z^T 2 [e_c]x R_B (Xi)
    or R_E 2 [e_c]x (Xj), chained through d(compact quaternion) / dR."""
    Rb, tb = iso_inv_mul(iso(xi), iso(xj))
    Rz, tz = iso(z)
    Re, te = Rz.T @ Rb, Rz.T @ (tb - tz)
    err = np.concatenate([te, R_to_quat(Re)[:3]])
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    Ji[:3, :3] = -Rz.T
    Jj[:3, :3] = Re
    Ji[:3, 3:] = Rz.T @ (2 * _skew(tb))
    D = _dq_dR(Re)
    for c in range(3):
        G = 2 * _skew(np.eye(3)[c])
        Mi, Mj = Rz.T @ (-G @ Rb), Re @ G
        Ji[3:, 3 + c] = np.einsum("krc,rc->k", D, Mi)
        Jj[3:, 3 + c] = np.einsum("krc,rc->k", D, Mj)
    return err, Ji, Jj


# ------------------------------------------------------------------------------------------ both
def between(d, xi, xj):
    return se3_between(xi, xj) if d == 6 else se2_between(xi, xj)


def edge(d, xi, xj, z):
    return se3_edge(xi, xj, z) if d == 6 else se2_edge(xi, xj, z)


def omega(d, upper):
    """row-wise upper triangle (the edge record of include/spg.h) -> full symmetric matrix"""
    om = np.zeros((d, d))
    om[np.triu_indices(d)] = upper
    return om + np.triu(om, 1).T


def upper(om):
    return np.asarray(om)[np.triu_indices(len(om))]


def error_covariance(d, xi, xj, z, Sigma_ab):
    """(e, J[D, 2D], P = J Sigma_ab J^T)"""
    e, Ji, Jj = edge(d, xi, xj, z)
    J = np.hstack([Ji, Jj])
    return e, J, J @ Sigma_ab @ J.T


def relative_covariance(d, xi, xj, Sigma_ab):
    """(rel, J, P) at z = the current relative pose"""
    rel = between(d, xi, xj)
    _, J, P = error_covariance(d, xi, xj, rel, Sigma_ab)
    return rel, J, P


def scores(e, P, Om):
    """(d2, gain, chi2) by the dense formulas of the header"""
    d = len(e)
    chi2 = float(e @ Om @ e)
    d2 = float(e @ np.linalg.solve(P + np.linalg.inv(Om), e))
    sign, ld = np.linalg.slogdet(np.eye(d) + Om @ P)
    return d2, (0.5 * ld if sign > 0 else np.nan), chi2


def compose(d, a, b):
    """a * b in the stored form (SE2: x y theta; SE3: t + unit quaternion with w >= 0)"""
    if d == 3:
        c, s = np.cos(a[2]), np.sin(a[2])
        return np.array([a[0] + c * b[0] - s * b[1], a[1] + s * b[0] + c * b[1], normalize_theta(a[2] + b[2])])
    Ra, ta = iso(a)
    Rb, tb = iso(b)
    return np.concatenate([ta + Ra @ tb, R_to_quat(Ra @ Rb)])


def from_mqt(v):
    """(t, compact quaternion) -> 7 stored numbers"""
    v = np.asarray(v, np.float64)
    return np.concatenate([v[:3], v[3:], [np.sqrt(max(0.0, 1.0 - v[3:] @ v[3:]))]])
