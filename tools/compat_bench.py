"""compatibleCandidates on the synthetic SE3 graph of the headline size: N candidates between two regions of the graph (two
blocks of --region consecutive vertices, so that the joint block stays inside its bound), a majority measured at the current
relative pose plus noise (mutually consistent), a group with one common offset and the rest with independent offsets, Omega
of an existing edge. One JSON line per call to stdout and appended to --out (diagnostic).

    python tools/compat_bench.py [--poses 100000] [--ring 400] [--candidates 2000] [--region 480] [--k 100] [--runs 5]
                                 [--out profiles/compat_100k_bench.jsonl]

pair_seconds, clique_seconds and verify_seconds are those of spg_compat_stats (HIP events around the per-candidate terms and
the pair tiles, the two clique kernels, the verify kernel); device_seconds and solve_seconds those of spg_cov_solve_stats
(factorisation, column solves, selected inverse, assembly and the three stages); covariance_seconds = device_seconds minus
the three stages. The same process times selectCandidates on the same candidates and k: it takes the same joint block, so its
device_seconds minus select_seconds stands beside covariance_seconds. The two calls alternate; medians over --runs calls
after one warm-up call each, min and max beside them. wall_seconds is the host clock around the whole call."""
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
ap.add_argument("--candidates", type=int, default=2000)
ap.add_argument("--region", type=int, default=480)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--inliers", type=float, default=0.6)
ap.add_argument("--aliased", type=float, default=0.2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compat_100k_bench.jsonl"))
args = ap.parse_args()

ctx = Context(0)
g = g2o_io.synth_sphere(args.poses, args.ring)
hg = GraphWrapperHIP.from_dict(g, ctx=ctx)
ids = hg.vertices()[0]
rng = np.random.default_rng(2024)
lo_a, lo_b = len(ids) // 4, (3 * len(ids)) // 4
A, B = ids[lo_a:lo_a + args.region], ids[lo_b:lo_b + args.region]
n = args.candidates
ij = np.stack([rng.choice(A, size=n), rng.choice(B, size=n)], axis=-1).astype(np.int32)
info = np.tile(g["edge_data"][0, 7:], (n, 1))
sig = 1.0 / np.sqrt(g["edge_data"][0, 7])               # the translation sigma of the generator's edges
meas = hg.relativeCovariances(ij)[0]                     # also the warm-up of the factorisation path
n_in, n_al = int(args.inliers * n), int(args.aliased * n)
meas[:, :3] += 0.5 * sig * rng.normal(size=(n, 3))
meas[n_in:n_in + n_al, :3] += 10.0 * sig * np.array([1.0, -0.7, 0.4])
meas[n_in + n_al:, :3] += 10.0 * sig * rng.normal(size=(n - n_in - n_al, 3))


def compat():
    return hg.compatibleCandidates(ij, meas, info, k=args.k, significance=0.99)


def select():
    return hg.selectCandidates(ij, meas, info, args.k, max_d2=got["max_d2"])


got = compat()                                           # warm-up: code objects, allocator
select()
keys_c = ("device_seconds", "solve_seconds", "pair_seconds", "clique_seconds", "verify_seconds")
keys_s = ("device_seconds", "solve_seconds", "select_seconds")
tc, ts = {k: [] for k in keys_c + ("wall_seconds",)}, {k: [] for k in keys_s + ("wall_seconds",)}
sc = ss = None
for _ in range(args.runs):
    t0 = time.perf_counter()
    got = compat()
    tc["wall_seconds"].append(time.perf_counter() - t0)
    sc = hg.last_covariance_stats
    for k in keys_c:
        tc[k].append(sc[k])
    t0 = time.perf_counter()
    sel = select()
    ts["wall_seconds"].append(time.perf_counter() - t0)
    ss = hg.last_covariance_stats
    for k in keys_s:
        ts[k].append(ss[k])
    print(f"compat: device {1e3 * tc['device_seconds'][-1]:.1f} ms (pairs {1e3 * sc['pair_seconds']:.2f}, set {1e3 * sc['clique_seconds']:.2f}, "
          f"gate {1e3 * sc['verify_seconds']:.2f}); select: device {1e3 * ts['device_seconds'][-1]:.1f} ms", file=sys.stderr, flush=True)


def spread(t, key):
    return {key: statistics.median(t[key]), key + "_min": min(t[key]), key + "_max": max(t[key])}


cov_c = [d - p - c - v for d, p, c, v in zip(tc["device_seconds"], tc["pair_seconds"], tc["clique_seconds"], tc["verify_seconds"])]
cov_s = [d - s for d, s in zip(ts["device_seconds"], ts["select_seconds"])]
line = {"workload": f"synthetic SE3, {args.poses} poses, ring {args.ring}: {n} candidates between two blocks of {args.region} vertices "
                    f"({n_in} consistent, {n_al} with a common offset, {n - n_in - n_al} independent)",
        "mode": "compat", "k": args.k, "candidates": n, "runs": args.runs, "endpoints": sc["endpoints"], "eligible": sc["eligible"],
        "consistent_pairs": sc["consistent_pairs"], "clique_size": sc["clique_size"], "seed": sc["seed"], "accepted": int(len(got["compatible"])),
        "accepted_outside_the_consistent_group": int((got["compatible"] >= n_in).sum()),
        **spread(tc, "pair_seconds"), **spread(tc, "clique_seconds"), **spread(tc, "verify_seconds"), **spread(tc, "device_seconds"),
        "solve_seconds": statistics.median(tc["solve_seconds"]), "wall_seconds": statistics.median(tc["wall_seconds"]),
        "covariance_seconds": statistics.median(cov_c), "covariance_seconds_min": min(cov_c), "covariance_seconds_max": max(cov_c),
        "select_covariance_seconds": statistics.median(cov_s), "select_covariance_seconds_min": min(cov_s), "select_covariance_seconds_max": max(cov_s),
        "select_seconds": statistics.median(ts["select_seconds"]), "select_device_seconds": statistics.median(ts["device_seconds"]),
        "select_wall_seconds": statistics.median(ts["wall_seconds"]), "select_endpoints": ss["endpoints"], "select_rounds": ss["rounds"],
        "selected_outside_the_consistent_group": int((sel["selected"] >= n_in).sum()),
        "columns": sc["columns"], "rhs_batches": sc["rhs_batches"], "supernodes": sc["supernodes"]}
text = json.dumps(line)
print(text, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    f.write(text + "\n")
