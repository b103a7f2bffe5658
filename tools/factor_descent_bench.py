"""Diagnostic: factor descent (SPG_FLAG_NFR_FACTOR_DESCENT, csrc/spg_nfr_fd.inc) against the interior point of the same
build on the blankets without a closed form. Not part of the product or the tests.

  sphere.g2o at full size (1 248 removals) under Subgraph(0.5)
  the hub of the 12-pose SE3 hub graph under Dense (tests/golden/digest_hub_dense_ip.npz is the oracle's result for it)
  the hub of a 23-pose SE3 hub graph under Dense (9 108 variables: beyond the interior point, SPG_ECAPACITY unflagged)

One JSON line per run, appended to profiles/factor_descent_bench.jsonl: wall and device time of marginalizeNoOptimize,
cycles (Newton steps for the interior point) per blanket, the sum of the per-blanket KLD, the global KLD of the result
against the input graph. The first call of a process pays the module load: every configuration runs once unrecorded
(--warmup 0 to skip; the unflagged 12-pose hub alone takes ~13 s)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsifyposegraph_amd import abi
from sparsifyposegraph_amd.graph import GraphWrapperHIP
from sparsifyposegraph_amd.lib import Context, SpgError
from tests import util
from tests.test_big_blankets import _star_graph


def run(ctx, name, g, which, topo, chord, fd):
    o = abi.make_options(g["pose_dim"], abi.ALG_NFR, topo, factor_descent=fd)
    o.chord_ratio = chord
    hg = GraphWrapperHIP.from_dict(g, ctx=ctx)
    rec = {"case": name, "solver": "factor descent" if fd else "interior point"}
    t0 = time.perf_counter()
    try:
        st = hg.marginalizeNoOptimize(which, o)
    except SpgError as e:
        rec.update(error=str(e)[:200])
        return rec
    wall = time.perf_counter() - t0
    b = hg.blankets()
    it = (b["info"] >> 8)[(b["info"] >> 8) > 0]
    base = GraphWrapperHIP.from_dict(g, ctx=ctx)
    fixed = next(int(v) for v in g["ids"] if int(v) not in set(int(w) for w in which))     # (the hub is vertex 0)
    rec.update(wall_s=round(wall, 4), device_s=round(st["device_seconds"], 4), removed=int(st["n_removed"]), bad_status=int(st["n_bad_status"]),
               blankets=int(len(it)), iterations_mean=round(float(it.mean()), 2) if len(it) else 0.0, iterations_max=int(it.max()) if len(it) else 0,
               at_max_cycles=int(((b["info"] & abi.INFO_FD_MAX_CYCLES) != 0).sum()), kld_sum=st["kld_sum"],
               global_kld=float(base.kullbackLeibler(hg, fixed)))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor_descent_bench.jsonl"))
    args = ap.parse_args()
    ctx = Context(0)
    sphere, which, *_ = util.load_golden("sphere_full_nfr_tree")
    hub = np.array([0], np.int32)
    cases = [("sphere.g2o Subgraph(0.5)", sphere, which, abi.TOPO_SUBGRAPH, 0.5),
             ("hub of 12 SE3 poses, Dense", _star_graph(12, seed=5), hub, abi.TOPO_DENSE, 1.0),
             ("hub of 23 SE3 poses, Dense", _star_graph(23, seed=5), hub, abi.TOPO_DENSE, 1.0)]
    with open(args.out, "a") as f:
        for case in cases:
            for fd in (True, False):
                for rep in range(args.warmup + 1):
                    rec = run(ctx, *case, fd)
                    if "error" in rec:
                        break
                if rec is not None:
                    line = json.dumps(rec)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()


if __name__ == "__main__":
    main()
