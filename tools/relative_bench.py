"""One vertex against all others on the synthetic SE3 graph of the headline size: scoreCandidates (candidates measured at
the current relative pose, Omega = the generator's info_diag), relativeCovariances, or pairCovariances of the same star
(the 2D x 2D blocks copied to the host: what a user had to start from before). One JSON line (diagnostic).

    python tools/relative_bench.py [--mode score|relative|pairs] [--poses 100000] [--ring 400] [--vertex 50000] [--runs 5]
    python tools/relative_bench.py --mode select --k K --candidates N [--endpoints 7000]
    python tools/relative_bench.py --mode prune --k K --candidates N --endpoints M
    python tools/relative_bench.py --mode outliers --k K --candidates N --endpoints M

--mode select: selectCandidates of N random pairs without a common edge, drawn over a random pool of at most --endpoints
(at most 7 000) vertices, Omega of an existing edge, z = the current relative pose plus noise; select_seconds, rounds and
endpoints are those of spg_select_stats. The same process also times one scoreCandidates call of the same list
(score_device_seconds): k of those, plus k addEdge and the round trips, is what the selection replaces.

--mode prune: pruneCandidates of up to N existing edges whose endpoints both fall in a block of M consecutive vertices
(every edge inside the block, at most N of them); prune_seconds, rounds and endpoints are those of spg_prune_stats. The
same process times selectCandidates at the same k on a list with the same endpoint pairs (z = the current relative pose
plus noise, Omega of an existing edge), so the column-solve part is the same and select_seconds stands beside prune_seconds.

--mode outliers: detectOutliers (no threshold: k rounds) of the candidate list of --mode prune at the generator's poses;
detect_seconds, rounds and endpoints are those of spg_outlier_stats. The rounds are the pruning's plus a D-vector per
candidate, so detect_seconds stands beside the prune_seconds of a --mode prune --skip-select run with the same arguments.

device_seconds and solve_seconds are those of spg_cov_solve_stats (HIP events: factorisation, column solves, selected
inverse, assembly and, for score / relative, sp_relative_kernel); wall_seconds is the host clock around the whole call
(plan, staging, uploads, the device work and the copy of the results). Medians over --runs calls after one warm-up call;
min and max are given beside them.

--method joint|lazy [--lookahead L] (select and prune): how the greedy call gets at Sigma (spg_ctx_set_greedy_method); the
line then carries spg_greedy_stats of the last run (method, lookahead, column_vertices, column_hits, rhs batches of the
rounds, round_solve_seconds, refactorised, cache_bytes). --skip-select (prune): do not time the selection twin, which
needs relativeCovariances of every candidate pair first."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsifyposegraph_amd import g2o_io  # noqa: E402
from sparsifyposegraph_amd.graph import GraphWrapperHIP  # noqa: E402
from sparsifyposegraph_amd.lib import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("score", "relative", "pairs", "select", "prune", "outliers"), default="score")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--candidates", type=int, default=2000)
ap.add_argument("--endpoints", type=int, default=7000)
ap.add_argument("--poses", type=int, default=100000)
ap.add_argument("--ring", type=int, default=400)
ap.add_argument("--vertex", type=int, default=50000)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--method", choices=("joint", "lazy"), default="joint")
ap.add_argument("--lookahead", type=int, default=0)
ap.add_argument("--skip-select", action="store_true")
args = ap.parse_args()

ctx = Context(0)
ctx.set_greedy_method({"joint": 0, "lazy": 1}[args.method], args.lookahead)


def greedy_extra():
    return {"method": args.method, **{"greedy_" + k: v for k, v in ctx.greedy_stats().items() if k != "method"}}


g = g2o_io.synth_sphere(args.poses, args.ring)
hg = GraphWrapperHIP.from_dict(g, ctx=ctx)
ids = hg.vertices()[0]
v0 = int(ids[min(args.vertex, len(ids) - 1)])
star = np.array([(v0, int(v)) for v in ids if int(v) != v0], np.int32)
if args.mode == "select":
    rng = np.random.default_rng(2024)
    pool = rng.choice(ids, size=min(args.endpoints, 7000, len(ids)), replace=False)
    adj = {(min(int(a), int(b)), max(int(a), int(b))) for a, b in g["edge_ij"]}
    far = []
    while len(far) < args.candidates:
        a, b = (int(x) for x in rng.choice(pool, size=2, replace=False))
        if (min(a, b), max(a, b)) not in adj:
            far.append((a, b))
    star = np.array(far, np.int32)
if args.mode in ("prune", "outliers"):
    lo = max(0, min(args.vertex, len(ids) - args.endpoints))
    pool = {int(v) for v in ids[lo:lo + args.endpoints]}
    e = hg.edges()
    inside = [k for k in range(len(e["kind"])) if all(int(v) in pool for v in e["vert_ids"][e["vert_off"][k]:e["vert_off"][k + 1]])]
    eidx = np.array(inside[:args.candidates], np.int32)
    star = np.array([e["vert_ids"][e["vert_off"][k]:e["vert_off"][k + 1]] for k in eidx], np.int32)
    rng = np.random.default_rng(2024)
    if args.mode == "prune" and not args.skip_select:
        meas = hg.relativeCovariances(star)[0]
        meas[:, :3] += 0.01 * rng.normal(size=(len(star), 3))
        info = np.tile(g["edge_data"][0, 7:], (len(star), 1))

    def timed(fn, key):
        fn()   # warm-up
        out = {"device": [], "solve": [], "wall": [], key: []}
        for _ in range(args.runs):
            t0 = time.perf_counter()
            r = fn()
            out["wall"].append(time.perf_counter() - t0)
            st = hg.last_covariance_stats
            out["device"].append(st["device_seconds"]); out["solve"].append(st["solve_seconds"]); out[key].append(st[key])
        return r, st, out
    med = statistics.median
    if args.mode == "outliers":
        ro, so, to = timed(lambda: hg.detectOutliers(eidx, args.k), "detect_seconds")
        print(json.dumps({
            "workload": f"synthetic SE3, {args.poses} poses, ring {args.ring}: {len(eidx)} existing edges inside a block of {len(pool)} vertices",
            "mode": "outliers", "k": args.k, "candidates": len(eidx), "runs": args.runs, "rounds": so["rounds"], "endpoints": so["endpoints"],
            "detect_seconds": med(to["detect_seconds"]), "detect_seconds_min": min(to["detect_seconds"]),
            "detect_seconds_max": max(to["detect_seconds"]),
            "device_seconds": med(to["device"]), "device_seconds_min": min(to["device"]), "device_seconds_max": max(to["device"]),
            "solve_seconds": med(to["solve"]), "wall_seconds": med(to["wall"]), "columns": so["columns"], "rhs_batches": so["rhs_batches"],
            "stat_first": float(ro["stat"][0]) if len(ro["stat"]) else 0.0, "stat_last": float(ro["stat"][-1]) if len(ro["stat"]) else 0.0,
            "untestable": int((ro["status"] == 2).sum()), **greedy_extra()}), flush=True)
        sys.exit(0)
    rp, sp, tp = timed(lambda: hg.pruneCandidates(eidx, args.k), "prune_seconds")
    gx = greedy_extra()
    if args.skip_select:
        print(json.dumps({
            "workload": f"synthetic SE3, {args.poses} poses, ring {args.ring}: {len(eidx)} existing edges inside a block of {len(pool)} vertices",
            "mode": "prune", "k": args.k, "candidates": len(eidx), "runs": args.runs, "rounds": sp["rounds"], "endpoints": sp["endpoints"],
            "prune_seconds": med(tp["prune_seconds"]), "prune_seconds_min": min(tp["prune_seconds"]), "prune_seconds_max": max(tp["prune_seconds"]),
            "device_seconds": med(tp["device"]), "device_seconds_min": min(tp["device"]), "device_seconds_max": max(tp["device"]),
            "solve_seconds": med(tp["solve"]), "wall_seconds": med(tp["wall"]), "columns": sp["columns"], "rhs_batches": sp["rhs_batches"],
            "kld": float(rp["kld"][-1]) if len(rp["kld"]) else 0.0, "bridges": int((rp["status"] == 2).sum()), **gx}), flush=True)
        sys.exit(0)
    rs, ss, ts = timed(lambda: hg.selectCandidates(star, meas, info, args.k), "select_seconds")
    print(json.dumps({
        "workload": f"synthetic SE3, {args.poses} poses, ring {args.ring}: {len(eidx)} existing edges inside a block of {len(pool)} vertices",
        "mode": "prune", "k": args.k, "candidates": len(eidx), "runs": args.runs, "rounds": sp["rounds"], "endpoints": sp["endpoints"],
        "prune_seconds": med(tp["prune_seconds"]), "prune_seconds_min": min(tp["prune_seconds"]), "prune_seconds_max": max(tp["prune_seconds"]),
        "device_seconds": med(tp["device"]), "device_seconds_min": min(tp["device"]), "device_seconds_max": max(tp["device"]),
        "solve_seconds": med(tp["solve"]), "wall_seconds": med(tp["wall"]), "columns": sp["columns"], "rhs_batches": sp["rhs_batches"],
        "kld": float(rp["kld"][-1]) if len(rp["kld"]) else 0.0, "bridges": int((rp["status"] == 2).sum()),
        "select_rounds": ss["rounds"], "select_endpoints": ss["endpoints"], "select_seconds": med(ts["select_seconds"]),
        "select_seconds_min": min(ts["select_seconds"]), "select_seconds_max": max(ts["select_seconds"]),
        "select_device_seconds": med(ts["device"]), "select_solve_seconds": med(ts["solve"]), "select_wall_seconds": med(ts["wall"]),
        "select_columns": ss["columns"], "prune_over_select": med(tp["prune_seconds"]) / med(ts["select_seconds"]), **gx}), flush=True)
    sys.exit(0)
info = np.tile(g["edge_data"][0, 7:], (len(star), 1))
meas = None
if args.mode == "select":
    meas = hg.relativeCovariances(star)[0]
    meas[:, :3] += 0.01 * rng.normal(size=(len(star), 3))
    score_dev = []
    for _ in range(2):                                  # the second call is the timed one
        hg.scoreCandidates(star, meas, info)
        score_dev.append(hg.last_covariance_stats["device_seconds"])
if args.mode == "score":
    meas = hg.relativeCovariances(star)[0]          # also the warm-up of the factorisation path


def call():
    if args.mode == "select":
        return sum(v.nbytes for v in hg.selectCandidates(star, meas, info, args.k).values())
    if args.mode == "score":
        return sum(v.nbytes for v in hg.scoreCandidates(star, meas, info).values())
    if args.mode == "relative":
        rel, cov = hg.relativeCovariances(star)
        return rel.nbytes + cov.nbytes
    return hg.pairCovariances(star).nbytes


call()   # warm-up: code objects, allocator
dev, solve, wall, nbytes, s, sel = [], [], [], 0, None, []
for _ in range(args.runs):
    t0 = time.perf_counter()
    nbytes = call()
    wall.append(time.perf_counter() - t0)
    s = hg.last_covariance_stats
    dev.append(s["device_seconds"])
    solve.append(s["solve_seconds"])
    sel.append(s.get("select_seconds", 0.0))
    print(f"{args.mode}: device {1e3 * dev[-1]:.1f} ms, wall {1e3 * wall[-1]:.1f} ms", file=sys.stderr, flush=True)
extra = {}
if args.mode == "select":
    extra = {"k": args.k, "rounds": s["rounds"], "endpoints": s["endpoints"], "select_seconds": statistics.median(sel),
             "select_seconds_min": min(sel), "select_seconds_max": max(sel), "score_device_seconds": score_dev[-1],
             "k_rescorings_device_seconds": args.k * score_dev[-1], **greedy_extra()}
what = f"vertex {v0} against all others" if args.mode != "select" else f"{len(star)} random far pairs over a pool of {len(pool)} vertices"
print(json.dumps({
    "workload": f"synthetic SE3, {args.poses} poses, ring {args.ring}: {what}", "mode": args.mode, **extra,
    "candidates": len(star), "columns": s["columns"], "rhs_batches": s["rhs_batches"], "runs": args.runs,
    "device_seconds": statistics.median(dev), "device_seconds_min": min(dev), "device_seconds_max": max(dev),
    "solve_seconds": statistics.median(solve), "wall_seconds": statistics.median(wall), "wall_seconds_min": min(wall),
    "wall_seconds_max": max(wall), "result_bytes": nbytes, "supernodes": s["supernodes"], "front_bytes": s["front_bytes"],
    "factor_flops": s["factor_flops"], "selinv_flops": s["selinv_flops"], "solve_flops": s["solve_flops"]}), flush=True)
