"""selectRemovals on the synthetic SE3 graph of the headline size. One JSON line per configuration to stdout and appended
to --out (diagnostic).

    python tools/removals_bench.py [--poses 100000] [--ring 400] [--radius 1.0] [--runs 5] [--chain-runs 2] [--chain-budget 60] [--no-host] [--host-only]
                                   [--out profiles/removals_100k_bench.jsonl]

Mode "select": no forced vertex, no angle test, at --radius (21 partners per vertex on the default graph) and at ten times
that (1 688), in hash order (priority None), "oldest" and "newest". device_seconds is spg_removal_stats' (HIP events from the
grid to the output: every round's launch and the host's read of the worklist size between two rounds are inside), wall_seconds
the host clock around the whole Python call (the order is sorted on the host, the call runs once); medians over --runs calls
after one warm-up, min and max beside them; rounds, n_kept and pairs_tested of the last call, the smallest and largest rounds
seen. The id-ordered chains need as many rounds as the trajectory is deep: a configuration whose first call takes more than a
second is repeated --chain-runs times only, and at the large radius an id order whose estimated device time exceeds
--chain-budget seconds is recorded as skipped with the estimate. Every line is appended to --out as it is measured.
Mode "propose" (the first yardstick): proposeCandidates stage A on the same graph and radius, min_id_gap 3, max_per_vertex 8,
in the same process.
Mode "host" (the second yardstick, what a caller could do before): the same rule in numpy on the host, vertex by vertex in
hash order against the kept set so far (one vectorised distance evaluation per vertex, O(n |K|) in all), on prefixes of the
trajectory of growing length until one takes more than --host-budget seconds; --host-only runs this alone, without a device.
Its n_kept at the full length is compared with the device's when both ran."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, default=100000)
ap.add_argument("--ring", type=int, default=400)
ap.add_argument("--radius", type=float, default=1.0)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--chain-runs", type=int, default=2)
ap.add_argument("--chain-budget", type=float, default=60.0)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--host-only", action="store_true")
ap.add_argument("--host-budget", type=float, default=60.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "removals_100k_bench.jsonl"))
args = ap.parse_args()

g = g2o_io.synth_sphere(args.poses, args.ring)
workload = f"synthetic SE3, {args.poses} poses, ring {args.ring}"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)


def emit(line):
    text = json.dumps(line)
    print(text, flush=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


def spread(v, key):
    return {key: statistics.median(v), key + "_min": min(v), key + "_max": max(v)}


def mix64(x):
    k = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        k = k ^ (k >> np.uint64(30)); k = k * np.uint64(0xbf58476d1ce4e5b9)
        k = k ^ (k >> np.uint64(27)); k = k * np.uint64(0x94d049bb133111eb)
        k = k ^ (k >> np.uint64(31))
    return k


def host_rule(ids, p, radius):
    """the sequential rule in hash order; returns (seconds, n_kept)"""
    t0 = time.perf_counter()
    order = np.lexsort((ids, mix64(ids.astype(np.uint32).astype(np.uint64))))
    kept = np.empty_like(p)
    nk = 0
    r2 = radius * radius
    for v in order:
        diff = kept[:nk] - p[v]
        if nk == 0 or not ((diff * diff).sum(axis=1) <= r2).any():
            kept[nk] = p[v]
            nk += 1
    return time.perf_counter() - t0, nk


device_kept = {}
if not args.host_only:
    from sparsifyposegraph_amd.graph import GraphWrapperHIP  # noqa: E402
    from sparsifyposegraph_amd.lib import Context  # noqa: E402
    hg = GraphWrapperHIP.from_dict(g, ctx=Context(0))
    n_live = hg.numVertices()
    per_round, chain_rounds = {}, 0
    for order in (None, "oldest", "newest"):
        for radius in (args.radius, 10.0 * args.radius):
            if order is not None and radius != args.radius:
                # the rounds of the chain at --radius times what a round of the hashed order costs here: an estimate, to keep
                # a run that would take many minutes out of the benchmark; it is recorded, not hidden
                estimate = chain_rounds * per_round[radius]
                if estimate > args.chain_budget:
                    emit({"workload": workload, "mode": "select", "radius": radius, "order": order, "skipped": True,
                          "estimated_device_seconds": estimate, "estimate": "rounds of this order at the small radius x device_seconds per round of "
                          "the hashed order at this radius"})
                    continue
            t0 = time.perf_counter()
            *_, s = hg.selectRemovals(radius, priority=order, stats=True)          # warm-up: code objects, allocator
            first = time.perf_counter() - t0
            runs = args.runs if first < 1.0 else args.chain_runs
            dev, wall, rounds = [], [], [s["rounds"]]
            for _ in range(runs):
                t0 = time.perf_counter()
                rem, rep, rd, s = hg.selectRemovals(radius, priority=order, stats=True)
                wall.append(time.perf_counter() - t0)
                dev.append(s["device_seconds"])
                rounds.append(s["rounds"])
            if order is None:
                device_kept[radius] = s["n_kept"]
                per_round[radius] = statistics.median(dev) / max(s["rounds"], 1)
            elif radius == args.radius:
                chain_rounds = max(chain_rounds, s["rounds"])
            emit({"workload": workload, "mode": "select", "radius": radius, "order": order or "hash", "runs": runs, "first_call_wall_seconds": first,
                  **spread(dev, "device_seconds"), **spread(wall, "wall_seconds"), "rounds": s["rounds"], "rounds_min": min(rounds),
                  "rounds_max": max(rounds), "device_seconds_per_round": statistics.median(dev) / max(s["rounds"], 1),
                  **{k: s[k] for k in ("n_live", "n_kept", "n_removed", "pairs_tested", "n_cells", "max_cell_population", "table_slots")},
                  "max_rep_dist": float(rd.max()) if len(rd) else 0.0})
    for radius in (args.radius, 10.0 * args.radius):
        kw = dict(min_id_gap=3, max_per_vertex=8, stats=True)
        got = hg.proposeCandidates(radius, **kw)
        dev, wall = [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            got = hg.proposeCandidates(radius, **kw)
            wall.append(time.perf_counter() - t0)
            dev.append(got["stats"]["device_seconds"])
        s = got["stats"]
        emit({"workload": workload, "mode": "propose", "radius": radius, "max_per_vertex": 8, "min_id_gap": 3, "runs": args.runs,
              **spread(dev, "device_seconds"), **spread(wall, "wall_seconds"), "pairs_tested": s["pairs_tested"], "n_kept": s["n_kept"],
              "partners_per_vertex": 2.0 * s["n_qualifying"] / n_live})

if not args.no_host:
    o = np.argsort(g["ids"])
    ids, p = np.asarray(g["ids"], np.int64)[o], np.ascontiguousarray(np.asarray(g["poses"], np.float64)[o][:, :3])
    for radius in (args.radius, 10.0 * args.radius):
        n = min(12500, len(ids))
        while True:
            seconds, nk = host_rule(ids[:n], p[:n], radius)
            line = {"workload": workload, "mode": "host", "what": "the sequential rule in numpy, hash order, a prefix of the trajectory", "radius": radius,
                    "n": n, "host_seconds": seconds, "n_kept": nk, "host_cpus": len(os.sched_getaffinity(0))}
            if n == len(ids) and radius in device_kept:
                line["device_n_kept"] = device_kept[radius]
            emit(line)
            if seconds > args.host_budget or n == len(ids):
                break
            n = min(2 * n, len(ids))
