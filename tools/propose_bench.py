"""proposeCandidates on the synthetic SE3 graph of the headline size. One JSON line per configuration to stdout and appended
to --out (diagnostic).

    python tools/propose_bench.py [--poses 100000] [--ring 400] [--radius 1.0] [--runs 5] [--no-brute]
                                  [--out profiles/propose_100k_bench.jsonl]

Stage A (mode "search"): every vertex a query, min_id_gap = 3, at --radius (of the order of ten partners per vertex on the
default graph: pose spacing 0.79 along a ring, 0.63 between rings) and at ten times that, with max_per_vertex 0 and 8.
device_seconds is spg_propose_stats' (HIP events around the stage-A kernels, the fill included), wall_seconds the host clock
around the whole Python call, which runs the search twice (the size query, then the fill) and copies the pairs back; medians
over --runs calls after one warm-up, min and max beside them.
The yardstick (mode "brute", the only thing a caller could do before): the same rule in numpy on the host, the distance
table in blocks of rows (|a|^2 + |b|^2 - 2 a.b through one matrix product per block), then the id gap, the common-edge test
and the cap on the pairs inside the radius; timed once, on this machine's CPUs. At ten times the radius only the blocked
distance table and its threshold are timed (the pairs inside, tens of millions, are counted, not kept). The brute-force pairs
at --radius are compared with the device's.
Stage B (mode "gate"): the last 1, 10 and 100 ids as the query list, range = 0.6 radius, z_max = 2: columns, solve_seconds and
device_seconds of spg_cov_solve_stats, beside relativeCovariances of the same pairs in the same process (the two alternate)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsifyposegraph_amd import g2o_io  # noqa: E402
from sparsifyposegraph_amd.graph import GraphWrapperHIP  # noqa: E402
from sparsifyposegraph_amd.lib import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, default=100000)
ap.add_argument("--ring", type=int, default=400)
ap.add_argument("--radius", type=float, default=1.0)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--gap", type=int, default=3)
ap.add_argument("--no-brute", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "propose_100k_bench.jsonl"))
args = ap.parse_args()

ctx = Context(0)
g = g2o_io.synth_sphere(args.poses, args.ring)
hg = GraphWrapperHIP.from_dict(g, ctx=ctx)
ids, poses = hg.vertices()
assert np.all(np.diff(ids) > 0)
workload = f"synthetic SE3, {args.poses} poses, ring {args.ring}"
lines = []


def emit(line):
    text = json.dumps(line)
    print(text, flush=True)
    lines.append(text)


def spread(v, key):
    return {key: statistics.median(v), key + "_min": min(v), key + "_max": max(v)}


def brute(radius, m, keep):
    """the rule on the host; keep = False: the blocked distance table and its threshold alone"""
    p = np.ascontiguousarray(poses[:, :3])
    n = len(p)
    sq = (p * p).sum(axis=1)
    edges = set()
    if keep:
        edges = {(min(int(a), int(b)), max(int(a), int(b))) for a, b in g["edge_ij"]}
    t0 = time.perf_counter()
    inside = 0
    rows, cols, dist = [], [], []
    block = 2000
    for lo in range(0, n, block):
        hi = min(lo + block, n)
        d2 = sq[lo:hi, None] + sq[None, :] - 2.0 * (p[lo:hi] @ p.T)
        a, b = np.nonzero(d2 <= radius * radius)
        inside += len(a)
        if keep:
            a += lo
            ok = (b > a) & (ids[b] - ids[a] >= args.gap)
            a, b = a[ok], b[ok]
            rows.append(a); cols.append(b); dist.append(np.sqrt(np.maximum(d2[a - lo, b], 0.0)))
    pairs = None
    if keep:
        a, b, dd = np.concatenate(rows), np.concatenate(cols), np.concatenate(dist)
        ok = np.array([(int(ids[x]), int(ids[y])) not in edges for x, y in zip(a, b)], bool)
        a, b, dd = a[ok], b[ok], dd[ok]
        if m > 0:
            # per vertex the m smallest (dist, partner id): both directions of every pair, one sort
            v = np.concatenate([a, b]); w = np.concatenate([b, a]); d2x = np.concatenate([dd, dd])
            o = np.lexsort((ids[w], d2x, v))
            v, w = v[o], w[o]
            first = np.r_[0, np.flatnonzero(np.diff(v)) + 1]
            rank = np.arange(len(v)) - np.repeat(first, np.diff(np.r_[first, len(v)]))
            pick = rank < m
            lo_, hi_ = np.minimum(v[pick], w[pick]), np.maximum(v[pick], w[pick])
            pairs = np.unique(np.stack([ids[lo_], ids[hi_]], axis=-1), axis=0)
        else:
            pairs = np.stack([ids[a], ids[b]], axis=-1)
            pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    return time.perf_counter() - t0, inside, pairs


# ------------------------------------------------------------------------------------------------------- stage A
for radius in (args.radius, 10.0 * args.radius):
    for m in (0, 8):
        kw = dict(min_id_gap=args.gap, max_per_vertex=m, stats=True)
        got = hg.proposeCandidates(radius, **kw)                       # warm-up: code objects, allocator
        dev, wall = [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            got = hg.proposeCandidates(radius, **kw)
            wall.append(time.perf_counter() - t0)
            dev.append(got["stats"]["device_seconds"])
        s = got["stats"]
        line = {"workload": workload, "mode": "search", "radius": radius, "max_per_vertex": m, "min_id_gap": args.gap, "runs": args.runs,
                **spread(dev, "device_seconds"), **spread(wall, "wall_seconds"),
                **{k: s[k] for k in ("pairs_tested", "n_qualifying", "n_kept", "n_cells", "max_cell_population", "table_slots")},
                "partners_per_vertex": 2.0 * s["n_qualifying"] / len(ids)}
        if not args.no_brute:
            keep = radius == args.radius
            seconds, inside, pairs = brute(radius, m, keep)
            line.update({"brute_seconds": seconds, "brute_what": "the whole rule" if keep else "the blocked distance table and its threshold alone",
                         "brute_inside_radius": int(inside), "brute_cpus": len(os.sched_getaffinity(0))})
            if keep:
                # the host forms |a|^2 + |b|^2 - 2 a.b: pairs within rounding of the radius or of a tau may differ
                mine, theirs = {tuple(x) for x in got["ij"].tolist()}, {tuple(x) for x in pairs.tolist()}
                line.update({"brute_pairs": len(theirs), "pairs_not_in_both": len(mine ^ theirs)})
        emit(line)

# ------------------------------------------------------------------------------------------------------- stage B
radius = args.radius
for nq in (1, 10, 100):
    q = [int(i) for i in ids[-nq:]]
    kw = dict(min_id_gap=args.gap, queries=q, range=0.6 * radius, z_max=2.0, stats=True)
    everything = hg.proposeCandidates(radius, min_id_gap=args.gap, queries=q, stats=True)
    pairs = everything["ij"]
    hg.proposeCandidates(radius, **kw)
    hg.relativeCovariances(pairs)
    tg = {k: [] for k in ("device_seconds", "solve_seconds", "wall_seconds", "search_seconds")}
    tr = {k: [] for k in ("device_seconds", "solve_seconds", "wall_seconds")}
    for _ in range(args.runs):
        t0 = time.perf_counter()
        got = hg.proposeCandidates(radius, **kw)
        tg["wall_seconds"].append(time.perf_counter() - t0)
        s = got["stats"]
        tg["device_seconds"].append(s["solve"]["device_seconds"]); tg["solve_seconds"].append(s["solve"]["solve_seconds"])
        tg["search_seconds"].append(s["device_seconds"])
        t0 = time.perf_counter()
        hg.relativeCovariances(pairs)
        tr["wall_seconds"].append(time.perf_counter() - t0)
        r = hg.last_covariance_stats
        tr["device_seconds"].append(r["device_seconds"]); tr["solve_seconds"].append(r["solve_seconds"])
    emit({"workload": workload, "mode": "gate", "radius": radius, "range": 0.6 * radius, "z_max": 2.0, "queries": nq, "runs": args.runs,
          "n_kept": s["n_kept"], "n_gated": s["n_gated"], "columns": s["solve"]["columns"], "rhs_batches": s["solve"]["rhs_batches"],
          **spread(tg["search_seconds"], "search_seconds"), **spread(tg["solve_seconds"], "solve_seconds"), **spread(tg["device_seconds"], "device_seconds"),
          **spread(tg["wall_seconds"], "wall_seconds"),
          "relative_columns": r["columns"], **spread(tr["solve_seconds"], "relative_solve_seconds"), **spread(tr["device_seconds"], "relative_device_seconds"),
          **spread(tr["wall_seconds"], "relative_wall_seconds")})

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    f.write("\n".join(lines) + "\n")
