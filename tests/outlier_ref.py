"""Plain numpy reference of the greedy data snooping (TEST HELPER, not product code): spg_graph_detect_outliers,
include/spg.h.

The linearised problem: chi2(x) = prior(x) + sum_j |e_j + A_j x|^2_Omega_j over the candidate edges j (select_ref.terms
gives A_j, Omega_j = L_j L_j^T, e_j and the column offsets), with x = 0 its minimiser and H its Hessian / 2 WITH every
candidate. Each round evaluates for every candidate that is not yet flagged, with F the flagged set, H_F = H - sum_F
A^T Omega A and x_F the minimiser without F,

    M_i    = I - L_i^T (A_i H_F^-1 A_i^T) L_i = G G^T     margin_i = the smallest squared pivot (prune_ref.pivots)
    e_i    = e_i(0) + A_i x_F
    stat_i = |G^-1 L_i^T e_i|^2 = e_i^T (Omega_i^-1 - A_i H_F^-1 A_i^T)^-1 e_i = min chi2 without F - min chi2 without F + i

takes the (largest statistic, lowest index) candidate among those with margin >= min_margin, and stops when that
statistic is below min_stat (> 0). `refit_greedy` is that literally, with one dense solve of the model per candidate and
round (it needs the prior: refit_model); `greedy_sigma` the same on Sigma = H^-1 with a Woodbury downdate of the whole
covariance and of x after each choice; `recurrence` the device's candidate-space algebra (per-candidate C_ii(t), e_i(t)
and histories B_i,s). Every round reports, per candidate, (stat, margin, lambda_min(M), |z|, ||L||), and every
conditioning (||K||, |w|, {i: ||B_i||}): the ingredients of the bound in tests/test_outlier_detection.py. Numpy only:
the GPU tests import this module.
"""
import numpy as np

from tests.prune_ref import _chol, _lam, pivots
from tests.select_ref import _support

INLIER, INFO_NOT_PD, UNTESTABLE, FLAGGED = 0, 1, 2, 3
MIN_MARGIN = 1e-6


def chi2_quantile(q, dof):
    """Wilson-Hilferty start, then Newton on the regularised incomplete gamma function by its power series (independent
    of abi.chi2_quantile: no bisection, no continued fraction); dof <= 6 and q <= 0.9999 keep the series short"""
    import math
    a = 0.5 * dof

    def P(x):
        term = total = 1.0 / a
        for n in range(1, 2000):
            term *= x / (a + n)
            total += term
        return total * math.exp(-x + a * math.log(x) - math.lgamma(a))
    z = np.sqrt(2.0) * _erfinv(2.0 * q - 1.0)
    x = dof * (1.0 - 2.0 / (9.0 * dof) + z * np.sqrt(2.0 / (9.0 * dof))) ** 3
    for _ in range(100):
        h = 0.5 * x
        pdf = math.exp(-h + (a - 1.0) * math.log(h) - math.lgamma(a)) * 0.5
        x -= (P(h) - q) / pdf
    return float(x)


def _erfinv(y):
    import math
    x = 0.0
    for _ in range(100):
        x -= (math.erf(x) - y) / (2.0 / math.sqrt(math.pi) * math.exp(-x * x))
    return x


def _stat(M, L, e, min_margin):
    """(stat or NaN, margin, lambda_min(M), |z|, ||L||) as the device evaluates a candidate"""
    ok, margin, _ = pivots(M, min_margin)
    z = L.T @ e
    stat = float(z @ np.linalg.solve(M, z)) if ok else np.nan
    return stat, margin, _lam(M), float(np.linalg.norm(z)), float(np.linalg.norm(L, 2))


def _run(n, k, usable, evaluate, condition, redundancy, min_stat, min_margin):
    """The greedy loop. evaluate(live) -> {i: (stat, margin, lambda_min, |z|, ||L||)}; condition(i) flags i and returns
    (||K||, |w|, {j: ||B_j||}). Returns a dict: flagged, stat, rounds, conds, final_stat, final_margin, final_lam,
    final_z, redundancy, status (n each)."""
    live = [i for i in range(n) if usable[i]]
    sel, cs, rounds, conds = [], [], [], []
    while len(sel) < k and live:
        ev = evaluate(live)
        rounds.append(ev)
        elig = [i for i in live if not np.isnan(ev[i][0]) and ev[i][1] >= min_margin]
        if not elig:
            break
        best = max(elig, key=lambda i: (ev[i][0], -i))
        if min_stat > 0 and ev[best][0] < min_stat:
            break
        sel.append(best)
        cs.append(ev[best][0])
        conds.append(condition(best))
        live.remove(best)
    out = {key: np.full(n, np.nan) for key in ("final_stat", "final_margin", "final_lam", "final_z")}
    status = np.array([INLIER if u else INFO_NOT_PD for u in usable], np.int32)
    status[sel] = FLAGGED
    if live:
        ev = evaluate(live)
        if len(rounds) == len(sel):
            rounds.append(ev)
        for i in live:
            out["final_margin"][i], out["final_lam"][i], out["final_z"][i] = ev[i][1], ev[i][2], ev[i][3]
            if not np.isnan(ev[i][0]) and ev[i][1] >= min_margin:
                out["final_stat"][i] = ev[i][0]
            else:
                status[i] = UNTESTABLE
    out.update({"flagged": np.array(sel, np.int32), "stat": np.array(cs), "rounds": rounds, "conds": conds,
                "redundancy": np.array(redundancy), "status": status})
    return out


def refit_model(H0, T):
    """A prior (x - c)^T H0 (x - c) that makes x = 0 the minimiser of prior + sum_j |e_j + A_j x|^2: H0 c = sum A^T Omega e"""
    return np.linalg.solve(H0, sum(t["A"].T @ t["Om"] @ t["e"] for t in T))


def refit(H0, c, T, keep):
    """Direct refit of the dense linear model with the edges in `keep`: (x, min chi2, H_keep)"""
    Hk = H0 + sum(T[j]["A"].T @ T[j]["Om"] @ T[j]["A"] for j in keep)
    x = np.linalg.solve(Hk, H0 @ c - sum(T[j]["A"].T @ T[j]["Om"] @ T[j]["e"] for j in keep))
    chi = (x - c) @ H0 @ (x - c) + sum((T[j]["e"] + T[j]["A"] @ x) @ T[j]["Om"] @ (T[j]["e"] + T[j]["A"] @ x) for j in keep)
    return x, float(chi), Hk


def refit_greedy(H0, c, T, usable, k, min_stat=0.0, min_margin=MIN_MARGIN):
    """The rule by direct refits: the statistic of i is the drop of the minimum chi2 when i is left out as well. Also
    returns `resid`: per round {i: e_i} at the refit without the flagged edges, and `chi2`: the minimum per round."""
    n, d = len(T), len(T[0]["e"])
    Lc = _chol(T, usable)
    st = {"keep": [j for j in range(n)], "resid": [], "chi2": []}
    S0 = np.linalg.inv(refit(H0, c, T, st["keep"])[2])
    red = [d - float(np.trace(Lc[i].T @ T[i]["A"] @ S0 @ T[i]["A"].T @ Lc[i])) if usable[i] else np.nan for i in range(n)]

    def evaluate(live):
        x, chi, Hk = refit(H0, c, T, st["keep"])
        out, res = {}, {}
        for i in live:
            A = T[i]["A"]
            e = T[i]["e"] + A @ x
            M = np.eye(d) - Lc[i].T @ A @ np.linalg.solve(Hk, A.T) @ Lc[i]
            s = list(_stat(M, Lc[i], e, min_margin))
            if not np.isnan(s[0]):
                s[0] = chi - refit(H0, c, T, [j for j in st["keep"] if j != i])[1]
            out[i], res[i] = tuple(s), e
        st["resid"].append(res)
        st["chi2"].append(chi)
        return out

    def condition(i):
        st["keep"].remove(i)
        return None
    out = _run(n, k, usable, evaluate, condition, red, min_stat, min_margin)
    out["resid"], out["chi2"] = st["resid"], st["chi2"]
    return out


def greedy_sigma(Sig, T, usable, k, min_stat=0.0, min_margin=MIN_MARGIN):
    """The same rule on the dense covariance: after each choice Sigma <- Sigma + Sigma A^T (Omega^-1 - P)^-1 A Sigma and
    x <- x + Sigma A^T (Omega^-1 - P)^-1 e over all N entries; e_i = e_i(0) + A_i x."""
    n, d = len(T), len(T[0]["e"])
    st = {"S": np.array(Sig, np.float64), "x": np.zeros(len(Sig))}
    sup = [_support(t, d) for t in T]
    Lc = _chol(T, usable)

    def P_of(i, s=None):
        idx, J = sup[i]
        if s is None:
            return J @ st["S"][np.ix_(idx, idx)] @ J.T
        return J @ st["S"][np.ix_(idx, sup[s][0])] @ sup[s][1].T

    def e_of(i):
        return T[i]["e"] + sup[i][1] @ st["x"][sup[i][0]]
    red = [d - float(np.trace(Lc[i].T @ P_of(i) @ Lc[i])) if usable[i] else np.nan for i in range(n)]
    chosen = set()

    def evaluate(live):
        return {i: _stat(np.eye(d) - Lc[i].T @ P_of(i) @ Lc[i], Lc[i], e_of(i), min_margin) for i in live}

    def condition(s):
        idx, J = sup[s]
        G = np.linalg.cholesky(np.eye(d) - Lc[s].T @ P_of(s) @ Lc[s])
        K = Lc[s] @ np.linalg.inv(G).T
        w = K.T @ e_of(s)
        nb = {i: float(np.linalg.norm(P_of(i, s) @ K, 2)) for i in range(n) if usable[i] and i not in chosen and i != s}
        SA = st["S"][:, idx] @ J.T                                   # Sigma A^T, N x D
        st["x"] = st["x"] + SA @ (K @ w)
        st["S"] = st["S"] + SA @ K @ K.T @ SA.T
        chosen.add(s)
        return float(np.linalg.norm(K, 2)), float(np.linalg.norm(w)), nb
    out = _run(n, k, usable, evaluate, condition, red, min_stat, min_margin)
    out["Sigma"], out["x"] = st["S"], st["x"]
    return out


def recurrence(Sig, T, usable, k, min_stat=0.0, min_margin=MIN_MARGIN):
    """The device's algebra in numpy: per candidate C_ii(t), e_i(t) and the history B_i,0..t-1; a round reads one cross
    block C_i*(0) per candidate from Sigma(0). M = I - L*^T C** L* = G G^T, K = L* G^-T, w = K^T e*, B_i,t = C_i*(t) K,
    C_ii += B B^T, e_i += B w. Also returns `resid`: per round {i: e_i(t)}."""
    n, d = len(T), len(T[0]["e"])
    sup = [_support(t, d) for t in T]
    Lc = _chol(T, usable)
    C = [sup[i][1] @ Sig[np.ix_(sup[i][0], sup[i][0])] @ sup[i][1].T for i in range(n)]
    e = [np.array(t["e"], np.float64) for t in T]
    red = [d - float(np.trace(Lc[i].T @ C[i] @ Lc[i])) if usable[i] else np.nan for i in range(n)]
    hist = [[] for _ in range(n)]
    chosen = set()
    resid = []

    def evaluate(live):
        resid.append({i: e[i].copy() for i in live})
        return {i: _stat(np.eye(d) - Lc[i].T @ C[i] @ Lc[i], Lc[i], e[i], min_margin) for i in live}

    def condition(s):
        G = np.linalg.cholesky(np.eye(d) - Lc[s].T @ C[s] @ Lc[s])
        K = Lc[s] @ np.linalg.inv(G).T
        w = K.T @ e[s]
        t = len(hist[s])
        live = [i for i in range(n) if usable[i] and i not in chosen]
        for i in live:
            X = sup[i][1] @ Sig[np.ix_(sup[i][0], sup[s][0])] @ sup[s][1].T
            for u in range(t):
                X = X + hist[i][u] @ hist[s][u].T
            hist[i].append(X @ K)
        for i in live:
            C[i] = C[i] + hist[i][t] @ hist[i][t].T
            if i != s:
                e[i] = e[i] + hist[i][t] @ w
        chosen.add(s)
        return float(np.linalg.norm(K, 2)), float(np.linalg.norm(w)), {i: float(np.linalg.norm(hist[i][t], 2)) for i in live if i != s}
    out = _run(n, k, usable, evaluate, condition, red, min_stat, min_margin)
    out["resid"] = resid
    return out


def one_shot(Sig, T, usable, min_stat, min_margin=MIN_MARGIN):
    """Indices whose round-0 statistic alone is >= min_stat: the test without re-conditioning"""
    ev = greedy_sigma(Sig, T, usable, 0, min_margin=min_margin)
    return [i for i in range(len(T)) if ev["final_stat"][i] >= min_stat]


# ------------------------------------------------------------------------------------------ the planted SE2 lattice
def lattice(side=6, n_planted=3, sigma=20.0, seed=7):
    """A side x side SE2 lattice (unit spacing, 4-neighbour edges: 2 side (side - 1) = 60 for side 6) read as a
    trajectory: the boustrophedon odometry chain (side^2 - 1 = 35 edges) and every other pair of lattice neighbours as a
    loop closure, 60 - 35 = 25 of them for side 6. Measurements carry unit-information noise
    scaled by 0.05; n_planted of the loop closures whose endpoints both have degree >= 3 get an extra offset of `sigma`
    standard deviations per component. Returns a graph dict (initial poses = the truth) and the planted edge indices."""
    from tests import relative_ref as rr
    rng = np.random.default_rng(seed)
    nv = side * side
    order = [(r, c if r % 2 == 0 else side - 1 - c) for r in range(side) for c in range(side)]
    vid = {rc: k for k, rc in enumerate(order)}
    truth = np.array([[c, r, 0.3 * rng.normal()] for r, c in order], np.float64)
    chain = [(k, k + 1) for k in range(nv - 1)]
    have = set(chain)
    nbrs = []
    for (r, c), k in vid.items():
        for rc in ((r + 1, c), (r, c + 1)):
            if rc in vid:
                a, b = sorted((k, vid[rc]))
                if (a, b) not in have:
                    nbrs.append((a, b))
    nbrs.sort()
    loops = nbrs
    ij = np.array(chain + loops, np.int32)
    std = 0.05
    info = np.eye(3) / std ** 2
    deg = np.bincount(ij.ravel(), minlength=nv)
    okl = [len(chain) + j for j, (a, b) in enumerate(loops) if deg[a] >= 3 and deg[b] >= 3]
    planted = sorted(int(x) for x in rng.choice(okl, size=n_planted, replace=False))
    meas = []
    for k, (a, b) in enumerate(ij):
        z = rr.between(3, truth[a], truth[b]) + std * rng.normal(size=3)
        if k in planted:
            z = z + sigma * std * rng.choice([-1.0, 1.0], size=3)
        meas.append(z)
    data = np.concatenate([np.array(meas), np.tile(rr.upper(info), (len(ij), 1))], axis=1)
    g = {"pose_dim": 3, "ids": np.arange(nv, dtype=np.int32), "poses": truth.copy(), "edge_ij": ij, "edge_data": data}
    return g, planted


def gauss_newton(g, poses, iters=30):
    """Gauss-Newton on the SE2 graph dict with vertex 0 fixed, numpy only: x <- x - H^-1 A^T Omega e on the tangent of
    relative_ref.edge (additive in (x, y, theta)). Returns the poses and the last step's norm."""
    from tests import select_ref as sr
    poses = np.array(poses, np.float64)
    ids = [int(i) for i in g["ids"]]
    at = {v: k for k, v in enumerate(ids[1:])}
    step = np.inf
    for _ in range(iters):
        T = sr.terms(3, {v: poses[k] for k, v in enumerate(ids)}, at, g["edge_ij"], g["edge_data"][:, :3], g["edge_data"][:, 3:])
        H = sum(t["A"].T @ t["Om"] @ t["A"] for t in T)
        b = sum(t["A"].T @ t["Om"] @ t["e"] for t in T)
        dx = -np.linalg.solve(H, b)
        poses[1:] += dx.reshape(-1, 3)
        step = float(np.linalg.norm(dx))
        if step < 1e-13:
            break
    return poses, step
