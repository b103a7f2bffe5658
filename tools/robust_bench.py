"""Cost of the robust kernels in optimize() on the synthetic SE3 graph of the headline size: device milliseconds per LM
iteration with the kernel off, with Huber and with DCS (every binary edge eligible), on the solver AUTO picks at that size
(block-sparse multifrontal). One JSON line per configuration.

    python tools/robust_bench.py [--poses 100000] [--ring 400] [--lm-iterations 3] [--runs 5] [--delta 1.0]

Each run stages a fresh copy of the graph, so every configuration starts from the same estimates; the per-iteration figure
is device_seconds of spg_optimize_stats over the LM iterations run. With a kernel set an iteration adds one pass of
edge_robust_kernel (and one of the n-ary Jacobian kernel when the graph has such edges) before the assembly and reads one
weight per binary edge in it; the iteration counts of the three configurations differ because the costs do."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsifyposegraph_amd import abi, g2o_io  # noqa: E402
from sparsifyposegraph_amd.graph import GraphWrapperHIP  # noqa: E402
from sparsifyposegraph_amd.lib import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, default=100000)
ap.add_argument("--ring", type=int, default=400)
ap.add_argument("--lm-iterations", type=int, default=3)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--delta", type=float, default=1.0)
args = ap.parse_args()

ctx = Context(0)
g = g2o_io.synth_sphere(args.poses, args.ring)
what = f"synthetic SE3, {args.poses} poses"
GraphWrapperHIP.from_dict(g, ctx=ctx).optimize(1)   # warm-up: code objects, allocator
for name, kind in (("off", abi.ROBUST_NONE), ("huber", abi.ROBUST_HUBER), ("dcs", abi.ROBUST_DCS)):
    per_it, st = [], None
    for _ in range(args.runs):
        h = GraphWrapperHIP.from_dict(g, ctx=ctx)
        h.setRobustKernel(kind, args.delta)
        st = h.optimize(args.lm_iterations)
        per_it.append(1e3 * st["device_seconds"] / max(st["iterations"], 1))
        if kind != abi.ROBUST_NONE:
            frac = float((h.edgeChi2()[2] < 1).mean())
        h.close()
    line = {"workload": what, "kernel": name, "delta": args.delta if kind else None, "solver": st["solver"], "n": st["n"],
            "lm_iterations": st["iterations"], "solves": st["trials"], "cost_initial": st["chi2_initial"], "cost_final": st["chi2_final"],
            "runs": args.runs, "device_ms_per_lm_iteration": statistics.median(per_it), "min": min(per_it), "max": max(per_it)}
    if kind != abi.ROBUST_NONE:
        line["down_weighted_fraction_final"] = frac
    print(json.dumps(line), flush=True)
