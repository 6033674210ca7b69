#!/usr/bin/env python3
"""Time the stages of the smoothed-aggregation setup (learnmultigrid_amd/aggregation.py, csrc/sa.hip) on an MI355X: on
jittered_poisson_2d(m) -- (m + 1)^2 nodes -- the symmetric strength pattern, the aggregation graph, the MIS-2 roots (with
their rounds), the two assignment phases, the tentative prolongator, the Jacobi step on it (its SpGEMM A T apart from the
merge), all of one level, and the whole sa_hierarchy down to max_coarse = 500 with its level sizes and complexities.  Next
to it, in the same process, amg.classical_hierarchy: its setup time and complexities, and for both hierarchies GMRES(10)
preconditioned by one V(2,2) damped-Jacobi (0.8) cycle to 1e-8 ||b||: iterations and time.  Each stage is warmed once; the
figure is the median of REPS runs, host clock around a device synchronise.  One JSON line per size.

It promises no number and asserts no ratio: whoever runs it writes the figures and the date into DESIGN.md and README.md.

Usage:  python tools/time_sa.py [elements per side ...]      (default 1024 2048: 1025^2 and 2049^2 nodes)"""
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
from learnmultigrid_amd.solvers import GMRES  # noqa: E402

DEV = "cuda:0"
REPS = 5
TARGET = 1e-8


def timed(f, reps=REPS):
    f()                                                   # warm: code objects, allocator
    ts, out = [], None
    for _ in range(reps):
        out = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def gmres(A, b, H):
    """(iterations, seconds, final residual / ||b||) of GMRES(10) with one V(2,2) damped-Jacobi cycle of H per iteration."""
    nb = float(np.linalg.norm(b))
    g = GMRES(A, b.reshape(-1, 1).copy())
    run = lambda: g.solve(max_iterations=300, error=TARGET * nb, restart=10, preconditioner=H, precond_steps=2, precond_omega=0.8)
    t, _ = timed(run, reps=3)
    return g.get_iterations(), round(t, 4), float(g.get_residual() / nb)


def device(m):
    A, b = P.jittered_poisson_2d(m)
    b = np.asarray(b, dtype=np.float64).ravel()
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    n = dA.shape[0]
    B = torch.ones(n, dtype=torch.float64, device=DEV)
    t_s, S = timed(lambda: agn.symmetric_strength_device(dA, 0.0))
    t_g, G = timed(lambda: agn.graph_device(S))
    t_mis, (state, rank, n_agg, rounds) = timed(lambda: agn.mis2_device(S, G))
    a1, a2 = (torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(2))
    t_assign, _ = timed(lambda: ops.sa_assign(G, state, rank, a1, a2))
    t_t, (T, Bc) = timed(lambda: agn.tentative_device(a2, n_agg, B))
    t_at, AT = timed(lambda: ops.spgemm(dA, T))
    rows = ops.sa_row_states(T)
    s = agn.jacobi_scale(dA)
    t_merge, P1 = timed(lambda: ops.amg_smooth(dA, T, AT, rows, rows, s, 0.0))
    t_level, _ = timed(lambda: agn.transfer_device(dA, B))
    out = {"elements_per_side": m, "nodes": n, "nnz": dA.nnz, "reps": REPS,
           "strength_s": round(t_s, 5), "graph_s": round(t_g, 5), "mis2_s": round(t_mis, 5), "mis2_rounds": rounds,
           "n_agg": n_agg, "assign_s": round(t_assign, 5), "tentative_s": round(t_t, 5), "spgemm_AT_s": round(t_at, 5),
           "jacobi_merge_s": round(t_merge, 5), "one_level_s": round(t_level, 5), "P_nnz": P1.nnz}
    del S, G, state, rank, a1, a2, T, Bc, AT, P1, rows
    for name, build in (("sa", lambda: agn.sa_hierarchy(dA, DEV)), ("classical", lambda: amg.classical_hierarchy(dA, DEV))):
        t_all, H = timed(build, reps=3)
        info = agn.hierarchy_info(H)
        its, t_solve, res = gmres(A, b, H)
        out[name] = {"hierarchy_s": round(t_all, 4), "level_sizes": H.sizes,
                     "operator_complexity": round(info["operator_complexity"], 3),
                     "grid_complexity": round(info["grid_complexity"], 3),
                     "gmres10_iterations": its, "gmres10_s": t_solve, "gmres10_residual": res,
                     "setup_plus_solve_s": round(t_all + t_solve, 4)}
        del H
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    del dA
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for m in [int(a) for a in sys.argv[1:]] or [1024, 2048]:
        device(m)
