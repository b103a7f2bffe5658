"""numpy formulas of the robust kernels of include/spg.h (SPG_ROBUST_*): rho(s) and the weight w = d rho / d s on
s = e^T Omega e >= 0, with width delta > 0."""
import numpy as np

NONE, HUBER, CAUCHY, GEMAN_MCCLURE, DCS = 0, 1, 2, 3, 4
KINDS = (HUBER, CAUCHY, GEMAN_MCCLURE, DCS)


def rho_w(kind, delta, s):
    """(rho, w) of every entry of s."""
    s = np.asarray(s, np.float64)
    d2 = delta * delta
    if kind == NONE:
        return s.copy(), np.ones_like(s)
    if kind == HUBER:
        big = s > d2
        r = np.sqrt(np.where(big, s, 1.0))
        return np.where(big, 2.0 * delta * r - d2, s), np.where(big, delta / r, 1.0)
    if kind == CAUCHY:
        t = s / d2
        return d2 * np.log1p(t), 1.0 / (1.0 + t)
    if kind == GEMAN_MCCLURE:
        a = d2 / (d2 + s)
        return a * s, a * a
    if kind == DCS:
        c = np.minimum(1.0, 2.0 * delta / (delta + s))
        u = 1.0 - c
        return c * c * s + delta * u * u, c * c
    raise ValueError(kind)
