"""Plain numpy reference of the greedy candidate selection by conditional information gain (TEST HELPER, not product
code): spg_graph_select_candidates, include/spg.h.

The rule, on the dense information H (the fixed vertex dropped, vertex v at columns at[v] D ... at[v] D + D): candidate i,
a hypothetical binary edge a -> b with Jacobians J = [Ja Jb] and error e of tests/relative_ref.py and information Omega,
has the full-width Jacobian A_i (D x N: Ja at a's columns, Jb at b's, nothing for the fixed vertex). Each round evaluates
for every eligible candidate

    gain_i = 1/2 (ln det(H + A_i^T Omega_i A_i) - ln det H)          np.linalg.slogdet on the dense matrices

picks the (largest gain, lowest index) candidate and adds its A^T Omega A to H. `greedy` is that, literally; it costs one
N^3 factorisation per candidate and round. `greedy_sigma` evaluates the same quantity on Sigma = H^-1 through the matrix
determinant lemma, 1/2 ln det(I + Omega A Sigma A^T) (the gain of relative_ref.scores), and rewrites the whole N x N
covariance after each choice (Woodbury), which is what makes the larger fixtures affordable; the tests hold the two
against each other. Neither uses the candidate-space recurrence of the device (per-candidate histories B_i,t), which
`recurrence` restates for the CPU test of the algebra. Numpy only: the GPU tests import this module.
"""
import numpy as np

from tests import relative_ref as rr


def terms(d, poses_of, at, ij, meas, info_upper):
    """Per candidate: (A[D, N] or None when Omega is unusable, Omega, e, J[D, 2D], (ca, cb)) with ca / cb the column
    offset of each endpoint in H or -1 for the fixed vertex. at: id -> block index in H (the fixed vertex absent)."""
    n_var = d * len(at)
    out = []
    for k, (a, b) in enumerate(ij):
        a, b = int(a), int(b)
        e, Ji, Jj = rr.edge(d, poses_of[a], poses_of[b], meas[k])
        Om = rr.omega(d, info_upper[k])
        A = np.zeros((d, n_var))
        cols = []
        for v, Jv in ((a, Ji), (b, Jj)):
            c = at[v] * d if v in at else -1
            cols.append(c)
            if c >= 0:
                A[:, c:c + d] = Jv
        ok = bool(np.all(np.isfinite(Om))) and np.linalg.eigvalsh(Om).min() > 0
        out.append({"A": A, "Om": Om, "e": e, "J": np.hstack([Ji, Jj]), "cols": tuple(cols), "ok": ok})
    return out


def _run(n, k, min_gain, eligible, gains_of, condition):
    """The greedy loop. gains_of(live) -> {i: gain}; condition(i) applies the choice. Returns a dict: selected, cond_gain,
    rounds (per round the gain of every candidate that was eligible in it), final_gain[n] (NaN unless still eligible)."""
    live = [i for i in range(n) if eligible[i]]
    sel, cg, rounds = [], [], []
    while len(sel) < k and live:
        g = gains_of(live)
        rounds.append(g)
        best = max(live, key=lambda i: (g[i], -i))
        if g[best] < min_gain:
            break
        sel.append(best)
        cg.append(g[best])
        condition(best)
        live.remove(best)
    final = np.full(n, np.nan)
    if live:
        g = gains_of(live)
        for i in live:
            final[i] = g[i]
    return {"selected": np.array(sel, np.int32), "cond_gain": np.array(cg), "rounds": rounds, "final_gain": final}


def greedy(H, T, eligible, k, min_gain=0.0):
    """The exact rule with slogdet on the dense information. T: terms(); eligible: bool per candidate."""
    st = {"H": np.array(H, np.float64)}

    def gains_of(live):
        ld0 = np.linalg.slogdet(st["H"])[1]
        return {i: 0.5 * (np.linalg.slogdet(st["H"] + T[i]["A"].T @ T[i]["Om"] @ T[i]["A"])[1] - ld0) for i in live}

    def condition(i):
        st["H"] = st["H"] + T[i]["A"].T @ T[i]["Om"] @ T[i]["A"]
    out = _run(len(T), k, min_gain, eligible, gains_of, condition)
    out["H"] = st["H"]
    return out


def _support(t, d):
    return np.concatenate([np.arange(c, c + d) for c in t["cols"] if c >= 0]), np.hstack([t["J"][:, s * d:(s + 1) * d] for s in (0, 1) if t["cols"][s] >= 0])


def greedy_sigma(Sig, T, eligible, k, min_gain=0.0):
    """The same rule on the dense covariance: gain = 1/2 ln det(I + Omega A Sigma A^T), and after each choice
    Sigma <- Sigma - Sigma A^T (Omega^-1 + A Sigma A^T)^-1 A Sigma over all N x N entries."""
    d = len(T[0]["e"])
    st = {"S": np.array(Sig, np.float64)}
    sup = [_support(t, d) for t in T]

    def P_of(i):
        idx, J = sup[i]
        return J @ st["S"][np.ix_(idx, idx)] @ J.T

    def gains_of(live):
        return {i: 0.5 * np.linalg.slogdet(np.eye(d) + T[i]["Om"] @ P_of(i))[1] for i in live}

    def condition(i):
        idx, J = sup[i]
        SA = st["S"][:, idx] @ J.T                                   # Sigma A^T, N x D
        st["S"] = st["S"] - SA @ np.linalg.solve(np.linalg.inv(T[i]["Om"]) + P_of(i), SA.T)
    return _run(len(T), k, min_gain, eligible, gains_of, condition)


def recurrence(Sig, T, eligible, k, min_gain=0.0):
    """The device's algebra in numpy: per candidate C_ii(t) and the history B_i,0..t-1; a round reads one cross block
    C_i*(0) per candidate from Sigma. Omega = L L^T, M = I + L*^T C** L* = G G^T, B_i,t = C_i*(t) L* G^-T."""
    d = len(T[0]["e"])
    n = len(T)
    sup = [_support(t, d) for t in T]
    Lc = [np.linalg.cholesky(t["Om"]) if eligible[i] else None for i, t in enumerate(T)]
    C = [sup[i][1] @ Sig[np.ix_(sup[i][0], sup[i][0])] @ sup[i][1].T for i in range(n)]
    hist = [[] for _ in range(n)]
    chosen = set()

    def gains_of(live):
        return {i: float(np.log(np.diag(np.linalg.cholesky(np.eye(d) + Lc[i].T @ C[i] @ Lc[i]))).sum()) for i in live}

    def condition(s):
        G = np.linalg.cholesky(np.eye(d) + Lc[s].T @ C[s] @ Lc[s])
        K = Lc[s] @ np.linalg.inv(G).T
        t = len(hist[s])
        live = [i for i in range(n) if eligible[i] and i not in chosen]      # s among them: later rounds read its entry
        for i in live:
            X = sup[i][1] @ Sig[np.ix_(sup[i][0], sup[s][0])] @ sup[s][1].T
            for u in range(t):
                X = X - hist[i][u] @ hist[s][u].T
            hist[i].append(X @ K)
        for i in live:
            C[i] = C[i] - hist[i][t] @ hist[i][t].T
        chosen.add(s)
    return _run(n, k, min_gain, eligible, gains_of, condition)
