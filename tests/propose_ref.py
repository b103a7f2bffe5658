"""Plain numpy reference of the candidate proposal (TEST HELPER, not product code): spg_graph_propose_candidates,
include/spg.h.

Stage A literally: the O(n^2) distance table, the five rules on it, the per-vertex cap through tau (the m-th smallest
(dist, partner id) of every query), the kept pairs in ascending (id_a, id_b) order. cells_tested counts what a grid with
cell edge = radius evaluates, the figure the device reports as pairs_tested. Stage B from a dense covariance through
tests/relative_ref.py: rho, sigma and zscore of one pair. Numpy only: the GPU tests import this module.
"""
import numpy as np

from tests import relative_ref as rr


def dim(d):
    return 3 if d == 6 else 2


def rotation_angle(d, xa, xb):
    """rotation angle of Xa^-1 Xb: SE2 |wrap(theta_b - theta_a)|, SE3 2 atan2(|vec|, |w|) of qa^-1 qb"""
    if d == 3:
        return abs(rr.normalize_theta(xb[2] - xa[2]))
    q = rr.se3_between(xa, xb)[3:]
    return 2.0 * np.arctan2(np.linalg.norm(q[:3]), abs(q[3]))


def distance_table(d, poses):
    p = np.asarray(poses, np.float64)[:, :dim(d)]
    diff = p[:, None, :] - p[None, :, :]
    s = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]
    if dim(d) == 3:
        s = s + diff[..., 2] * diff[..., 2]
    return np.sqrt(s)


def qualifying(d, ids, poses, adjacent, radius, max_angle=0.0, min_id_gap=1, queries=None):
    """Rules 1 to 5. ids ascending; adjacent: set of (id_a, id_b), id_a < id_b, with a common live edge. Returns
    {(a, b): (dist, angle)} over positions a < b in ids."""
    ids = [int(i) for i in ids]
    assert ids == sorted(ids)
    n = len(ids)
    isq = np.ones(n, bool) if queries is None else np.isin(ids, [int(q) for q in queries])
    dist = distance_table(d, poses)
    out = {}
    for a in range(n):
        for b in np.flatnonzero(dist[a] <= radius):
            b = int(b)
            if b <= a or not (isq[a] or isq[b]):
                continue
            if min_id_gap > 1 and ids[b] - ids[a] < min_id_gap:
                continue
            if (ids[a], ids[b]) in adjacent:
                continue
            ang = rotation_angle(d, poses[a], poses[b])
            if max_angle > 0 and not ang <= max_angle:
                continue
            out[(a, b)] = (float(dist[a, b]), float(ang))
    return out, isq


def propose(d, ids, poses, adjacent, radius, max_angle=0.0, min_id_gap=1, m=0, queries=None):
    """Stage A. Returns a dict: ij int32[n, 2] (ids), dist, angle, n_qualifying, partners (per position, the sorted
    (dist, id) lists of the queries: the tie checks of the tests read them)."""
    ids = [int(i) for i in ids]
    qual, isq = qualifying(d, ids, poses, adjacent, radius, max_angle, min_id_gap, queries)
    partners = {v: [] for v in range(len(ids)) if isq[v]}
    for (a, b), (dist, _) in qual.items():
        if isq[a]:
            partners[a].append((dist, ids[b]))
        if isq[b]:
            partners[b].append((dist, ids[a]))
    tau = {}
    for v, lst in partners.items():
        lst.sort()
        tau[v] = lst[m - 1] if 0 < m <= len(lst) else (np.inf, np.iinfo(np.int32).max)
    kept = [(a, b) for (a, b), (dist, _) in qual.items()
            if (isq[a] and (dist, ids[b]) <= tau[a]) or (isq[b] and (dist, ids[a]) <= tau[b])]
    kept.sort()
    return {"ij": np.array([(ids[a], ids[b]) for a, b in kept], np.int32).reshape(-1, 2),
            "dist": np.array([qual[k][0] for k in kept]), "angle": np.array([qual[k][1] for k in kept]),
            "n_qualifying": len(qual), "partners": partners, "qualifying": qual}


def cells_tested(positions, radius, queries=None):
    """The exact number of (query, partner) evaluations of a grid with cell edge = radius over the 3^dim cells around
    every query, partner != query. queries: a boolean mask or positions into `positions`; None: everybody."""
    p = np.asarray(positions, np.float64)
    n, k = p.shape
    cell = np.floor(p / radius).astype(np.int64)
    count = {}
    for c in map(tuple, cell):
        count[c] = count.get(c, 0) + 1
    q = np.arange(n) if queries is None else np.arange(n)[np.asarray(queries)]
    offsets = np.array(np.meshgrid(*[[-1, 0, 1]] * k, indexing="ij")).reshape(k, -1).T
    total = 0
    for v in q:
        total += sum(count.get(tuple(cell[v] + o), 0) for o in offsets) - 1
    return int(total)


def gate(d, xa, xb, Sigma_ab, rng):
    """Stage B of one pair: (rho, sigma, zscore, J, P) with P = J Sigma_ab J^T at the current relative pose, u = R_z^T t_z / rho,
    sigma^2 = u^T P_tt u, zscore = (rho - range) / sigma (sigma = 0: -inf when rho <= range, else +inf)"""
    k = dim(d)
    rel, J, P = rr.relative_covariance(d, xa, xb, Sigma_ab)
    t = rel[:k]
    rho = float(np.linalg.norm(t))
    if d == 3:
        c, s = np.cos(rel[2]), np.sin(rel[2])
        Rz = np.array([[c, -s], [s, c]])
    else:
        Rz = rr.quat_to_R(rel[3:])
    u = Rz.T @ t / rho if rho > 0 else np.eye(k)[0]
    s2 = max(float(u @ P[:k, :k] @ u), 0.0)
    sg = np.sqrt(s2)
    if sg > 0:
        z = (rho - rng) / sg
    else:
        z = -np.inf if rho <= rng else np.inf
    return rho, sg, z, J, P
