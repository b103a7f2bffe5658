"""Plain numpy reference of the selection of removals (TEST HELPER, not product code): spg_graph_select_removals,
include/spg.h.

The rule literally: the redundancy relation on tests/propose_ref.py's distance_table and rotation_angle, the total order
(the keep list, then priority descending / the hashed id ascending, ties to the id), the sequential greedy pass that builds the
lexicographically first maximal independent set, the representative of every removed vertex. `rounds` replays the same
rule in synchronous rounds, each reading only the verdicts of the round before, and returns the number of rounds it took:
the dependency depth of the order, an upper bound of the launches the device needs. Numpy only: the GPU tests import this
module.
"""
import numpy as np

from tests import propose_ref as pr

U64 = np.uint64


def mix64(x):
    """the splitmix64 finaliser on np.uint64 (scalar or array), all 64 bits kept"""
    k = np.asarray(x, dtype=U64)
    with np.errstate(over="ignore"):
        k = k ^ (k >> U64(30))
        k = k * U64(0xbf58476d1ce4e5b9)
        k = k ^ (k >> U64(27))
        k = k * U64(0x94d049bb133111eb)
        k = k ^ (k >> U64(31))
    return k


def redundancy(d, poses, radius, max_angle=0.0):
    """(boolean n x n table of "redundant with", the distance table); positions in ascending-id order, the angle asked with
    the lower position first"""
    dist = pr.distance_table(d, poses)
    red = dist <= radius
    np.fill_diagonal(red, False)
    if max_angle > 0:
        for a, b in zip(*np.nonzero(np.triu(red))):
            if not pr.rotation_angle(d, poses[a], poses[b]) <= max_angle:
                red[a, b] = red[b, a] = False
    return red, dist


def priority_values(ids, priority):
    """the per-vertex doubles of "oldest" / "newest" / a dict / an array; None stays None"""
    if priority is None:
        return None
    if isinstance(priority, str):
        return np.asarray(ids, np.float64) * (-1.0 if priority == "oldest" else 1.0)
    if isinstance(priority, dict):
        return np.array([priority[int(i)] for i in ids], np.float64)
    return np.asarray(priority, np.float64)


def order_of(ids, keep=(), priority=None):
    """positions (into the ascending ids) in the total order, and the number forced"""
    ids = [int(i) for i in ids]
    assert ids == sorted(ids)
    at = {v: i for i, v in enumerate(ids)}
    forced = [at[int(k)] for k in keep]
    assert len(set(forced)) == len(forced)
    rest = [i for i in range(len(ids)) if i not in set(forced)]
    p = priority_values(ids, priority)
    if p is None:
        h = mix64(np.array(ids, np.int64).astype(np.uint32).astype(U64))
        rest.sort(key=lambda i: (int(h[i]), ids[i]))
    else:
        assert not np.isnan(p).any()
        rest.sort(key=lambda i: (-p[i], ids[i]))
    return forced + rest, len(forced)


def sequential(red, order, n_forced):
    """the kept mask of the rule: the forced, then every vertex in order that no kept vertex is redundant with"""
    kept = np.zeros(len(order), bool)
    kept[order[:n_forced]] = True
    for v in order[n_forced:]:
        if not (red[v] & kept).any():
            kept[v] = True
    return kept


def rounds(red, order, n_forced):
    """(kept mask, depth): synchronous rounds over the undecided vertices, each from the verdicts of the round before:
    removed iff an earlier redundant vertex is kept, kept iff all of them are removed"""
    n = len(order)
    place = np.empty(n, np.int64)
    place[order] = np.arange(n)
    state = np.zeros(n, np.int8)                      # 0 undecided, 1 kept, 2 removed
    state[order[:n_forced]] = 1
    earlier = [np.flatnonzero(red[v] & (place < place[v])) for v in range(n)]
    depth = 0
    while (state == 0).any():
        new = state.copy()
        for v in np.flatnonzero(state == 0):
            s = state[earlier[v]]
            if (s == 1).any():
                new[v] = 2
            elif (s == 2).all():
                new[v] = 1
        assert (new != state).any()
        state = new
        depth += 1
    return state == 1, depth


def select(d, ids, poses, radius, max_angle=0.0, keep=(), priority=None, table=None):
    """The whole call by the sequential rule. ids ascending; table: redundancy(...) of the same arguments, computed once by
    a caller that asks several orders. Returns a dict: removed, representative (int32 ids, removed ascending), rep_dist,
    kept (mask over positions), red, dist, order, n_forced."""
    ids = [int(i) for i in ids]
    red, dist = redundancy(d, poses, radius, max_angle) if table is None else table
    order, nf = order_of(ids, keep, priority)
    kept = sequential(red, order, nf)
    removed, rep, rd = [], [], []
    for v in np.flatnonzero(~kept):
        cand = np.flatnonzero(red[v] & kept)
        best = min(cand, key=lambda u: (dist[v, u], ids[u]))
        removed.append(ids[v]); rep.append(ids[best]); rd.append(dist[v, best])
    return {"removed": np.array(removed, np.int32), "representative": np.array(rep, np.int32), "rep_dist": np.array(rd, np.float64),
            "kept": kept, "red": red, "dist": dist, "order": order, "n_forced": nf}
