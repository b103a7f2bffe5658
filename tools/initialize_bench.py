"""initialize() on the synthetic SE3 graph of the headline size, from identity poses: time of both modes and how many
LM iterations optimize() needs afterwards. One JSON line per mode (diagnostic; no bar is set on these figures).

    python tools/initialize_bench.py [--poses 100000] [--ring 400] [--runs 3] [--lm-iterations 50]

Every estimate but the first is reset to the identity, so each run starts from what addVertex / addEdge users have.
device_ms is device_seconds of spg_init_stats (HIP events around assembly, both factorisations, the solves and the
projection; 0 for the spanning tree, which runs on the host); call_ms is the host clock around the whole call (it adds
the plan, the staging, chi2 before and after and the download of the poses). The LM that follows runs once per mode; its
reference is optimize() from the generator's ground-truth poses."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsifyposegraph_amd import abi, g2o_io  # noqa: E402
from sparsifyposegraph_amd.graph import GraphWrapperHIP  # noqa: E402
from sparsifyposegraph_amd.lib import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, default=100000)
ap.add_argument("--ring", type=int, default=400)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--lm-iterations", type=int, default=50)
args = ap.parse_args()

ctx = Context(0)
g = g2o_io.synth_sphere(args.poses, args.ring)
what = f"synthetic SE3, {args.poses} poses, ring {args.ring}"
blank = np.array(g["poses"], float).copy()
blank[1:] = [0, 0, 0, 0, 0, 0, 1.0]
lost = dict(g, poses=blank)

ref = GraphWrapperHIP.from_dict(g, ctx=ctx)
want = ref.optimize(args.lm_iterations)
ref.close()
GraphWrapperHIP.from_dict(lost, ctx=ctx).initialize(abi.INIT_CHORDAL)   # warm-up: code objects, allocator
for name, method in (("spanning_tree", abi.INIT_SPANNING_TREE), ("chordal", abi.INIT_CHORDAL)):
    dev, call, st, h = [], [], None, None
    for _ in range(args.runs):
        if h is not None:
            h.close()
        h = GraphWrapperHIP.from_dict(lost, ctx=ctx)
        h.chi2()   # the graph is on the device before the clock starts
        t0 = time.perf_counter()
        st = h.initialize(method)
        call.append(1e3 * (time.perf_counter() - t0))
        print(f"{name}: call {call[-1]:.1f} ms", file=sys.stderr, flush=True)
        dev.append(1e3 * st["device_seconds"])
    lm = h.optimize(args.lm_iterations)
    h.close()
    print(json.dumps({
        "workload": what, "method": name, "n_vertices": st["n_vertices"], "edges_used": st["edges_used"], "tree_depth": st["tree_depth"],
        "degenerate": st["degenerate"], "supernodes": st["supernodes"], "front_bytes": st["front_bytes"], "factor_flops": st["factor_flops"],
        "chi2_identity": st["chi2_before"], "chi2_initialized": st["chi2_after"], "runs": args.runs,
        "device_ms": statistics.median(dev), "device_ms_min": min(dev), "device_ms_max": max(dev),
        "call_ms": statistics.median(call), "call_ms_min": min(call), "call_ms_max": max(call),
        "lm_iterations_after": lm["iterations"], "lm_solves_after": lm["trials"], "lm_chi2_final": lm["chi2_final"],
        "lm_device_ms": 1e3 * lm["device_seconds"], "lm_chi2_final_from_ground_truth": want["chi2_final"],
        "lm_iterations_from_ground_truth": want["iterations"]}), flush=True)
