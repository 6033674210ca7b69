#!/usr/bin/env python3
"""Time the K-cycle on an MI355X (learnmultigrid_amd/hierarchy.py: Hierarchy.cycle(shape="K"); csrc/krylov.hip).

steps   The two inner steps (ops.kcycle_step1 / kcycle_step2, k_inner "gcr") in their one-launch and two-launch forms over
        n = 2^10 .. 2^22: microseconds per step from a captured graph of CHAIN step-1 / step-2 pairs (what a cycle replays)
        and from the same chain launched eagerly, median of REPS windows after a warm-up.  The last line names the largest
        power of two at which the one-launch form is no slower than the two-launch form for BOTH steps in the graph: what
        kKcOneLaunchMax in csrc/krylov.hip should be.
solves  GMRES(10) preconditioned by one V-, W- or K-shaped (2,2) damped-Jacobi (0.8) cycle to 1e-8 |b| on
        jittered_poisson_2d(m), on the smoothed-aggregation and the classical hierarchy (and the geometric one where the
        grid has one): iterations, solve time, setup + solve time, median of REPS warm runs in one process.

It promises no number and asserts no ratio: whoever runs it writes the figures and the date into DESIGN.md and README.md.
One JSON line per measurement.

Usage:  python tools/time_kcycle.py steps
        python tools/time_kcycle.py solves [elements per side ...]      (default 1024 2048: 1025^2 and 2049^2 nodes)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from learnmultigrid_amd import aggregation as agn, amg, ops, problems as P  # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy  # noqa: E402
from learnmultigrid_amd.solvers import GMRES  # noqa: E402

DEV = "cuda:0"
REPS = 5
CHAIN = 50
TARGET = 1e-8


def median_seconds(f, reps=REPS):
    f()                                                   # warm: code objects, allocator
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def steps():
    g = torch.Generator().manual_seed(5)
    stream = torch.cuda.Stream(DEV)
    best = None
    with torch.cuda.stream(stream):
        for e in range(10, 23):
            n = 1 << e
            c1, v1, b, c2, v2 = (torch.rand(n, dtype=torch.float64, generator=g).to(DEV) - 0.5 for _ in range(5))
            rt, x = torch.zeros_like(b), torch.zeros_like(b)
            scal = torch.zeros(len(ops.KCYCLE_SCALARS), dtype=torch.float64, device=DEV)
            part = torch.zeros(ops.kcycle_partials_count(n), dtype=torch.float64, device=DEV)
            row = {"n": n, "grid": ops.kcycle_grid(n), "chain": CHAIN, "reps": REPS}
            for form in ("one", "two"):
                s1 = lambda: ops.kcycle_step1("gcr", c1, v1, b, rt, scal, part, form=form)              # noqa: E731
                s2 = lambda: ops.kcycle_step2("gcr", c1, v1, c2, v2, rt, scal, x, part, form=form)      # noqa: E731
                for name, call in (("step1", s1), ("step2", s2)):
                    def chain():
                        for _ in range(CHAIN):
                            call()
                    graph = ops.CapturedGraph()
                    with graph:
                        chain()
                    row["%s_%s_graph_us" % (name, form)] = round(1e6 * median_seconds(graph.launch) / CHAIN, 2)
                    row["%s_%s_eager_us" % (name, form)] = round(1e6 * median_seconds(chain) / CHAIN, 2)
                    del graph
            row["one_launch_no_slower"] = all(row["%s_one_graph_us" % s] <= row["%s_two_graph_us" % s] for s in ("step1", "step2"))
            if row["one_launch_no_slower"]:
                best = n
            print(json.dumps(row), flush=True)
    print(json.dumps({"largest_power_of_two_with_one_launch_no_slower": best,
                      "library_constant": ops.kcycle_one_launch_max()}), flush=True)


def gmres(A, b, H, shape, k_inner="gcr"):
    nb = float(np.linalg.norm(b))
    g = GMRES(A, b.reshape(-1, 1).copy())
    run = lambda: g.solve(max_iterations=400, error=TARGET * nb, restart=10, preconditioner=H, precond_steps=2,   # noqa: E731
                          precond_omega=0.8, precond_cycle_shape=shape, precond_k_inner=k_inner)
    t = median_seconds(run)
    return g.get_iterations(), t, float(g.get_residual() / nb)


def solves(m):
    A, b = P.jittered_poisson_2d(m)
    b = np.asarray(b, dtype=np.float64).ravel()
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    levels = max(2, int(np.log2(m)) - 3)
    builders = [("sa", lambda: agn.sa_hierarchy(dA, DEV)), ("classical", lambda: amg.classical_hierarchy(dA, DEV)),
                ("geometric", lambda: Hierarchy(A, P.geometric_hierarchy_2d(m + 1, levels), DEV))]
    for name, build in builders:
        build()
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            H = build()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        setup = statistics.median(ts)
        for shape, k_inner in (("V", None), ("W", None), ("K", "gcr"), ("K", "fcg")):
            its, t, res = gmres(A, b, H, shape, k_inner or "gcr")
            print(json.dumps({"elements_per_side": m, "nodes": dA.shape[0], "hierarchy": name, "level_sizes": H.sizes,
                              "setup_s": round(setup, 4), "cycle": shape, "k_inner": k_inner, "gmres10_iterations": its,
                              "solve_s": round(t, 4), "setup_plus_solve_s": round(setup + t, 4), "residual": res,
                              "reps": REPS}), flush=True)
        del H
        torch.cuda.empty_cache()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "steps":
        steps()
    elif what == "solves":
        for m in [int(a) for a in sys.argv[2:]] or [1024, 2048]:
            solves(m)
    else:
        sys.exit(__doc__)
