"""Measurement target of the block-CSR information (csrc/spg_bsr.inc) on the synthetic SE3 graph of the headline size:
assembly into block-CSR next to the assembly into the sparse solver's fronts, the product H x (time, bytes moved, rate
against the HBM peak) and optimize() by PCG next to the sparse Cholesky, per linear solve. Prints JSON lines.

    python tools/bsr_bench.py [--poses 100000] [--ring 400] [--reps 50] [--lm-iterations 3]

The bytes of one product are what the algorithm has to move: every block and its column index once, x and y once. The
matrix (144 MB at 100 000 poses) fits the 256 MiB Infinity Cache, so repeated products are served from there: the rate is
reported against the HBM peak for comparison, not as HBM traffic."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsifyposegraph_amd import abi, g2o_io  # noqa: E402
from sparsifyposegraph_amd.graph import GraphWrapperHIP  # noqa: E402
from sparsifyposegraph_amd.lib import Context, check  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E, spec

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, default=100000)
ap.add_argument("--ring", type=int, default=400)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--lm-iterations", type=int, default=3)
args = ap.parse_args()

ctx = Context(0)
g = g2o_io.synth_sphere(args.poses, args.ring)
what = f"synthetic SE3, {args.poses} poses"
hg = GraphWrapperHIP.from_dict(g, ctx=ctx)
D, nb = 6, args.poses - 1
fn = hg.L.spg_debug_bsr_bench
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_int, C.POINTER(C.c_double)]
out = np.zeros(4)
check(fn(hg.h, -1, args.reps, out.ctypes.data_as(C.POINTER(C.c_double))), ctx.h, "spg_debug_bsr_bench")
asm_ms, spmv_ms, front_ms, nnzb = float(out[0]), float(out[1]), float(out[2]), int(out[3])
spmv_bytes = nnzb * (D * D * 8 + 4) + (nb + 1) * 8 + 2 * nb * D * 8
gbs = spmv_bytes / (spmv_ms * 1e-3) / 1e9
print(json.dumps({"workload": what, "measure": "assembly", "reps": args.reps, "blocks": nnzb, "value_MB": nnzb * D * D * 8 / 1e6,
                  "bsr_assembly_ms": asm_ms, "front_assembly_ms": front_ms}))
print(json.dumps({"workload": what, "measure": "H x (bsr_spmv_kernel)", "reps": args.reps, "ms": spmv_ms, "bytes": spmv_bytes, "GB_per_s": gbs,
                  "hbm_peak_GB_per_s": HBM_PEAK_GBS, "frac_of_hbm_peak": gbs / HBM_PEAK_GBS,
                  "note": "back-to-back products of a matrix that fits the Infinity Cache"}))

for name, solver in (("pcg", abi.SOLVER_PCG), ("sparse", abi.SOLVER_SPARSE)):
    ctx.set_linear_solver(solver)
    h2 = GraphWrapperHIP.from_dict(g, ctx=ctx)
    t0 = time.perf_counter()
    st = h2.optimize(args.lm_iterations)
    wall = time.perf_counter() - t0
    ps = ctx.pcg_stats()
    line = {"workload": what, "measure": f"optimize({args.lm_iterations}) with {name}", "n": st["n"], "lm_iterations": st["iterations"], "solves": st["trials"],
            "chi2_initial": st["chi2_initial"], "chi2_final": st["chi2_final"], "device_seconds": st["device_seconds"], "wall_seconds": wall,
            "device_seconds_per_solve": st["device_seconds"] / max(st["trials"], 1)}
    if solver == abi.SOLVER_PCG:
        line.update(cg_iterations=ps["iterations"], cg_iterations_per_solve=ps["iterations"] / max(ps["solves"], 1), unconverged=ps["unconverged"],
                    last_rel_residual=ps["last_rel_residual"], solve_seconds_per_solve=ps["solve_seconds"] / max(ps["solves"], 1),
                    ms_per_cg_iteration=1e3 * ps["solve_seconds"] / max(ps["iterations"], 1))
    print(json.dumps(line))
    h2.close()
ctx.set_linear_solver(abi.SOLVER_AUTO)
