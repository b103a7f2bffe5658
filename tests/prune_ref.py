"""Plain numpy reference of the greedy edge pruning by conditional information loss (TEST HELPER, not product code):
spg_graph_prune_candidates, include/spg.h.

The rule, on the dense information H of the graph WITH all its edges (the fixed vertex dropped; select_ref.terms gives
the full-width Jacobian A_i, Omega_i = L_i L_i^T and the column offsets of every candidate, an existing binary edge): each
round evaluates for every candidate that is not yet pruned

    M_i      = I - L_i^T (A_i H^-1 A_i^T) L_i = G G^T     margin_i = the smallest squared pivot of that factorisation
    loss_i   = 1/2 (ln det H - ln det(H - A_i^T Omega_i A_i)) = -1/2 ln det M_i

takes the (smallest loss, lowest index) candidate among those with margin >= min_margin and subtracts its A^T Omega A
from H. `greedy` is that with slogdet on the dense matrices, `greedy_sigma` the same on Sigma = H^-1 with a Woodbury
downdate of the whole covariance after each choice, `recurrence` the device's candidate-space algebra (per-candidate
C_ii(t) and histories B_i,s). All three report the per-round margins and the cumulative KLD by the closed form
kld(t) = sum loss_s - 1/2 sum tr(Omega_s A_s Sigma(0) A_s^T). Numpy only: the GPU tests import this module.
"""
import numpy as np

from tests.select_ref import _support

KEPT, INFO_NOT_PD, BRIDGE, PRUNED = 0, 1, 2, 3
MIN_MARGIN = 1e-6


def pivots(M, min_margin):
    """Cholesky of M as the device runs it: stops at the first squared pivot that is not finite, <= 0 or below
    min_margin. Returns (ok, margin = smallest squared pivot seen, loss = -sum log G_jj or NaN)."""
    M = np.array(M, np.float64)
    d = len(M)
    margin, loss = np.inf, 0.0
    for j in range(d):
        p = M[j, j] - M[j, :j] @ M[j, :j]
        if not np.isfinite(p):
            return False, np.nan, np.nan
        margin = min(margin, p)
        if not p > 0.0 or p < min_margin:
            return False, margin, np.nan
        g = np.sqrt(p)
        M[j, j] = g
        loss -= np.log(g)
        for r in range(j + 1, d):
            M[r, j] = (M[r, j] - M[r, :j] @ M[j, :j]) / g
    return True, margin, loss


def _run(n, k, usable, evaluate, condition, tr0, max_loss, max_kld, min_margin):
    """The greedy loop. evaluate(live) -> {i: (loss, margin, lambda_min(M_i))}; condition(i) applies the removal. Returns a dict: pruned,
    cond_loss, kld (cumulative), rounds (per round {i: (loss, margin, lambda_min)} of every candidate not yet pruned), final_loss,
    final_margin, final_lam (lambda_min(M_i) after the last round), status (n each)."""
    live = [i for i in range(n) if usable[i]]
    sel, cl, ck, rounds = [], [], [], []
    kld = 0.0
    while len(sel) < k and live:
        ev = evaluate(live)
        rounds.append(ev)
        elig = [i for i in live if not np.isnan(ev[i][0]) and ev[i][1] >= min_margin]
        if not elig:
            break
        best = min(elig, key=lambda i: (ev[i][0], i))
        loss = ev[best][0]
        if max_loss > 0 and loss > max_loss:
            break
        new = kld + (loss - 0.5 * tr0[best])
        if max_kld > 0 and new > max_kld:
            break
        kld = new
        sel.append(best)
        cl.append(loss)
        ck.append(kld)
        condition(best)
        live.remove(best)
    final_loss, final_margin, final_lam = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    status = np.array([KEPT if u else INFO_NOT_PD for u in usable], np.int32)
    status[sel] = PRUNED
    if live:
        ev = evaluate(live)
        for i in live:
            final_margin[i], final_lam[i] = ev[i][1], ev[i][2]
            if not np.isnan(ev[i][0]) and ev[i][1] >= min_margin:
                final_loss[i] = ev[i][0]
            else:
                status[i] = BRIDGE
    return {"pruned": np.array(sel, np.int32), "cond_loss": np.array(cl), "kld": np.array(ck), "rounds": rounds,
            "final_loss": final_loss, "final_margin": final_margin, "final_lam": final_lam, "status": status}


def _lam(M):
    """smallest eigenvalue of the symmetric part of M"""
    return float(np.linalg.eigvalsh(0.5 * (M + M.T)).min())


def _chol(T, usable):
    return [np.linalg.cholesky(t["Om"]) if usable[i] else None for i, t in enumerate(T)]


def greedy(H, T, usable, k, max_loss=0.0, max_kld=0.0, min_margin=MIN_MARGIN):
    """The rule by slogdet on the dense information. T: select_ref.terms() of the edges; usable: Omega is PD."""
    st = {"H": np.array(H, np.float64)}
    Lc = _chol(T, usable)
    S0 = np.linalg.inv(st["H"])
    tr0 = [float(np.trace(t["Om"] @ t["A"] @ S0 @ t["A"].T)) if usable[i] else np.nan for i, t in enumerate(T)]

    def evaluate(live):
        out = {}
        ld0 = np.linalg.slogdet(st["H"])[1]
        for i in live:
            A = T[i]["A"]
            M = np.eye(len(A)) - Lc[i].T @ A @ np.linalg.solve(st["H"], A.T) @ Lc[i]
            ok, margin, _ = pivots(M, min_margin)
            loss = np.nan
            if ok:
                sign, ld = np.linalg.slogdet(st["H"] - A.T @ T[i]["Om"] @ A)
                loss = 0.5 * (ld0 - ld) if sign > 0 else np.nan
            out[i] = (loss, margin, _lam(M))
        return out

    def condition(i):
        st["H"] = st["H"] - T[i]["A"].T @ T[i]["Om"] @ T[i]["A"]
    out = _run(len(T), k, usable, evaluate, condition, tr0, max_loss, max_kld, min_margin)
    out["H"] = st["H"]
    return out


def greedy_sigma(Sig, T, usable, k, max_loss=0.0, max_kld=0.0, min_margin=MIN_MARGIN):
    """The same rule on the dense covariance: M = I - L^T P L with P = A Sigma A^T, and after each choice
    Sigma <- Sigma + Sigma A^T (Omega^-1 - P)^-1 A Sigma over all N x N entries."""
    d = len(T[0]["e"])
    st = {"S": np.array(Sig, np.float64)}
    sup = [_support(t, d) for t in T]
    Lc = _chol(T, usable)

    def P_of(i):
        idx, J = sup[i]
        return J @ st["S"][np.ix_(idx, idx)] @ J.T
    tr0 = [float(np.trace(T[i]["Om"] @ P_of(i))) if usable[i] else np.nan for i in range(len(T))]

    def evaluate(live):
        out = {}
        for i in live:
            M = np.eye(d) - Lc[i].T @ P_of(i) @ Lc[i]
            ok, margin, loss = pivots(M, min_margin)
            out[i] = (loss, margin, _lam(M))
        return out

    def condition(i):
        idx, J = sup[i]
        SA = st["S"][:, idx] @ J.T                                   # Sigma A^T, N x D
        st["S"] = st["S"] + SA @ np.linalg.solve(np.linalg.inv(T[i]["Om"]) - P_of(i), SA.T)
    out = _run(len(T), k, usable, evaluate, condition, tr0, max_loss, max_kld, min_margin)
    out["Sigma"] = st["S"]
    return out


def recurrence(Sig, T, usable, k, max_loss=0.0, max_kld=0.0, min_margin=MIN_MARGIN):
    """The device's algebra in numpy: per candidate C_ii(t) and the history B_i,0..t-1; a round reads one cross block
    C_i*(0) per candidate from Sigma(0). M = I - L*^T C** L* = G G^T, B_i,t = C_i*(t) L* G^-T, C_ii += B B^T."""
    d = len(T[0]["e"])
    n = len(T)
    sup = [_support(t, d) for t in T]
    Lc = _chol(T, usable)
    C = [sup[i][1] @ Sig[np.ix_(sup[i][0], sup[i][0])] @ sup[i][1].T for i in range(n)]
    tr0 = [float(np.trace(Lc[i].T @ C[i] @ Lc[i])) if usable[i] else np.nan for i in range(n)]
    hist = [[] for _ in range(n)]
    chosen = set()

    def evaluate(live):
        out = {}
        for i in live:
            M = np.eye(d) - Lc[i].T @ C[i] @ Lc[i]
            ok, margin, loss = pivots(M, min_margin)
            out[i] = (loss, margin, _lam(M))
        return out

    def condition(s):
        G = np.linalg.cholesky(np.eye(d) - Lc[s].T @ C[s] @ Lc[s])
        K = Lc[s] @ np.linalg.inv(G).T
        t = len(hist[s])
        live = [i for i in range(n) if usable[i] and i not in chosen]
        for i in live:
            X = sup[i][1] @ Sig[np.ix_(sup[i][0], sup[s][0])] @ sup[s][1].T
            for u in range(t):
                X = X + hist[i][u] @ hist[s][u].T
            hist[i].append(X @ K)
        for i in live:
            C[i] = C[i] + hist[i][t] @ hist[i][t].T
        chosen.add(s)
    return _run(n, k, usable, evaluate, condition, tr0, max_loss, max_kld, min_margin)


def kld_trace_logdet(H, Hp):
    """1/2 (tr(Hp H^-1) - N + ln det H - ln det Hp): the KLD of the pruned graph against the original, mean term 0"""
    n = len(H)
    return 0.5 * (np.trace(Hp @ np.linalg.inv(H)) - n + np.linalg.slogdet(H)[1] - np.linalg.slogdet(Hp)[1])


def connectivity_bridges(n_vertices, edges):
    """Indices of the edges (a, b) (vertex numbers 0 .. n_vertices - 1, parallel edges allowed) whose removal disconnects
    the multigraph: the lowpoint rule on a depth-first tree, iterative."""
    adj = [[] for _ in range(n_vertices)]
    for k, (a, b) in enumerate(edges):
        adj[a].append((b, k))
        adj[b].append((a, k))
    disc, low = [-1] * n_vertices, [0] * n_vertices
    out, clock = [], 0
    for root in range(n_vertices):
        if disc[root] >= 0:
            continue
        disc[root] = low[root] = clock
        clock += 1
        stack = [(root, -1, iter(adj[root]))]
        while stack:
            v, pe, it = stack[-1]
            step = next(it, None)
            if step is None:
                stack.pop()
                if stack:
                    u = stack[-1][0]
                    low[u] = min(low[u], low[v])
                    if low[v] > disc[u]:
                        out.append(pe)
                continue
            w, k = step
            if k == pe:
                continue
            if disc[w] >= 0:
                low[v] = min(low[v], disc[w])
            else:
                disc[w] = low[w] = clock
                clock += 1
                stack.append((w, k, iter(adj[w])))
    return sorted(out)
