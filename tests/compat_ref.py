"""Plain numpy reference of the joint compatibility of candidates (TEST HELPER, not product code):
spg_graph_compatible_candidates and spg_ctx_max_clique, include/spg.h.

With the terms of tests/select_ref.py (candidate i: full-width Jacobian A_i, information Omega_i, error e_i) and the dense
covariance Sigma of the gauge, the joint distance of a set S is computed literally as

    d2(S) = e_S^T (blockdiag(Omega_i^-1) + A_S Sigma A_S^T)^-1 e_S          np.linalg.inv, np.linalg.solve

which forms Omega^-1; the device never does (it works on M = I + L^T (A Sigma A^T) L with Omega = L L^T). The stages:

  eligible   Omega usable, and d2({i}) <= max_d2 when max_d2 > 0
  stage 1    every unordered eligible pair: d2({i, j}) <= pair_max_d2 (not finite: inconsistent) -> a symmetric boolean
             matrix with a clear diagonal
  stage 2    greedy_clique: for every eligible seed s, R = [s], P = N(s); while P: v = the u in P with the most neighbours
             in P (ties: the lowest index), R += [v], P &= N(v); the longest R, ties to the lowest seed
  stage 3    the members in ascending (d2_i, index); S = [], and member i is accepted iff there are no thresholds or
             d2(S + [i]) <= joint_max_d2[len(S)]; stop after k acceptances

`pair_by_elimination` restates the device's D x D route (i eliminated first) for the CPU test of the algebra; `bound` is the
error bound of a set's distance derived in tests/test_candidate_compatibility.py. Numpy only: the GPU tests import this.
"""
import numpy as np

SCORED, INFO_NOT_PD, GATED, SELECTED, INCOMPATIBLE = 0, 1, 2, 3, 4


def dense_d2(T, Sig, S):
    """d2(S), literally. T: select_ref.terms(); S: candidate indices."""
    S = list(S)
    d = len(T[S[0]]["e"])
    A = np.vstack([T[i]["A"] for i in S])
    e = np.concatenate([T[i]["e"] for i in S])
    C = A @ Sig @ A.T
    for k, i in enumerate(S):
        C[k * d:(k + 1) * d, k * d:(k + 1) * d] += np.linalg.inv(T[i]["Om"])
    return float(e @ np.linalg.solve(C, e))


def _uw(t):
    L = np.linalg.cholesky(t["Om"])
    return L.T @ t["A"], L.T @ t["e"]


def pair_by_elimination(T, Sig, i, j):
    """The device's route in numpy: d2_i + |G^-1 (w_j - M_ji M_ii^-1 w_i)|^2, G G^T = M_jj - M_ji M_ii^-1 M_ij."""
    d = len(T[i]["e"])
    Ui, wi = _uw(T[i])
    Uj, wj = _uw(T[j])
    Mii, Mij, Mjj = np.eye(d) + Ui @ Sig @ Ui.T, Ui @ Sig @ Uj.T, np.eye(d) + Uj @ Sig @ Uj.T
    Gi = np.linalg.cholesky(Mii)
    x = np.linalg.solve(Gi, wi)
    X = np.linalg.solve(Gi, Mij)
    G = np.linalg.cholesky(Mjj - X.T @ X)
    y = np.linalg.solve(G, wj - X.T @ x)
    return float(x @ x + y @ y)


def sequential_by_cholesky(T, Sig, order):
    """The device's stage-3 recurrence in numpy, without thresholds: d2 of every prefix of `order` by the left-looking block
    Cholesky of M_SS."""
    d = len(T[order[0]]["e"])
    U, w = zip(*[_uw(T[i]) for i in order])
    G = np.zeros((len(order) * d, len(order) * d))
    y = np.zeros(len(order) * d)
    out, D2 = [], 0.0
    for p in range(len(order)):
        row = np.hstack([U[p] @ Sig @ U[s].T for s in range(p)]) if p else np.zeros((d, 0))
        GiS = np.linalg.solve(G[:p * d, :p * d], row.T).T if p else row
        Gii = np.linalg.cholesky(np.eye(d) + U[p] @ Sig @ U[p].T - GiS @ GiS.T)
        yi = np.linalg.solve(Gii, w[p] - GiS @ y[:p * d])
        G[p * d:(p + 1) * d, :p * d], G[p * d:(p + 1) * d, p * d:(p + 1) * d], y[p * d:(p + 1) * d] = GiS, Gii, yi
        D2 += float(yi @ yi)
        out.append(D2)
    return np.array(out)


def bound(T, Sig, S):
    """The derived bound on |d2(S) - reference| (module docstring of the test): |w_S|^2 |S| D max ||Omega||2 beta."""
    S = list(S)
    d = len(T[S[0]]["e"])
    scale = float(np.abs(Sig).max())
    jn = {i: np.abs(T[i]["J"]).sum(axis=1).max() for i in S}
    beta = 0.0
    for a, i in enumerate(S):
        for j in S[a:]:
            beta = max(beta, jn[i] * jn[j] * 1e-9 * scale + 1e-11 * np.abs(T[i]["A"] @ Sig @ T[j]["A"].T).max())
    w2 = sum(float(T[i]["e"] @ T[i]["Om"] @ T[i]["e"]) for i in S)
    return w2 * len(S) * d * max(np.linalg.norm(T[i]["Om"], 2) for i in S) * beta


def greedy_clique(adj, eligible=None):
    """Stage 2 on a boolean matrix (symmetric, clear diagonal). Returns (members in order of construction, seed);
    ([], -1) when nothing is eligible."""
    adj = np.asarray(adj, bool)
    n = len(adj)
    best, best_seed = [], -1
    for s in range(n):
        if eligible is not None and not eligible[s]:
            continue
        R, P = [s], adj[s].copy()
        while P.any():
            cnt = (adj & P[None, :]).sum(axis=1)
            cand = np.flatnonzero(P)
            v = int(cand[np.argmax(cnt[cand])])      # argmax returns the first maximum: the lowest index
            R.append(v)
            P &= adj[v]
        if len(R) > len(best):
            best, best_seed = R, s
    return best, best_seed


def run(T, Sig, k, max_d2, pair_max_d2, joint_max_d2=None):
    """The three stages. Returns a dict: d2[n], eligible[n], pair_d2[n, n] (diagonal d2_i, NaN for ineligible), adj, degree,
    clique, seed, order (the members in stage-3 order), compatible, joint_d2, tested (per member examined: (i, t, |S|,
    accepted)), status[n]."""
    n = len(T)
    d2 = np.full(n, np.nan)
    status = np.zeros(n, np.int32)
    for i, t in enumerate(T):
        if not t["ok"]:
            status[i] = INFO_NOT_PD
            continue
        d2[i] = dense_d2(T, Sig, [i])
        if max_d2 > 0 and not d2[i] <= max_d2:
            status[i] = GATED
    elig = status == SCORED
    pd = np.full((n, n), np.nan)
    adj = np.zeros((n, n), bool)
    for i in range(n):
        if not elig[i]:
            continue
        pd[i, i] = d2[i]
        for j in range(i + 1, n):
            if elig[j]:
                pd[i, j] = pd[j, i] = dense_d2(T, Sig, [i, j])
                adj[i, j] = adj[j, i] = bool(pd[i, j] <= pair_max_d2)
    clique, seed = greedy_clique(adj, elig)
    order = sorted(clique, key=lambda i: (d2[i], i))
    S, jd, tested = [], [], []
    for i in order:
        if len(S) >= k:
            break
        t = dense_d2(T, Sig, S + [i])
        ok = bool(np.isfinite(t)) and (joint_max_d2 is None or t <= joint_max_d2[len(S)])
        tested.append((i, t, len(S), ok))
        if ok:
            S.append(i)
            jd.append(t)
            status[i] = SELECTED
        else:
            status[i] = INCOMPATIBLE
    return {"d2": d2, "eligible": elig, "pair_d2": pd, "adj": adj, "degree": adj.sum(axis=1).astype(np.int32), "clique": clique, "seed": seed,
            "order": order, "compatible": np.array(S, np.int32), "joint_d2": np.array(jd), "tested": tested, "status": status}
