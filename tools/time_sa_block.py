#!/usr/bin/env python3
"""Time smoothed aggregation for systems (learnmultigrid_amd/aggregation.py, csrc/nsp.hip) on an MI355X: on elasticity_2d(m)
-- (m + 1)^2 nodes, two unknowns each -- the stages of the fine level (condensation, strength, aggregates, the tentative
prolongator of the three rigid-body modes, the Jacobi step on it), and the whole sa_hierarchy down to max_coarse = 500 with
its level sizes and complexities for three choices of candidates, in the same process: the rigid-body modes on node blocks
of 2, the two translations alone (block_size=2, B=None), and today's scalar setup with a vector of ones.  For each of the
three, CG preconditioned by one V(2,2) damped-Jacobi (0.5) cycle and GMRES(20) preconditioned by one K-cycle
(k_inner="fcg") of the same smoothing, to 1e-8 ||b|| or MAX_ITERATIONS: iterations and time.  Each stage is warmed once; the
figure is the median of REPS runs, host clock around a device synchronise.  One JSON line per size.

It promises no number and asserts no ratio: whoever runs it writes the figures and the date into DESIGN.md and README.md.

Usage:  python tools/time_sa_block.py [elements per side ...]      (default 1024 2048: 1025^2 and 2049^2 nodes)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from learnmultigrid_amd import aggregation as agn, ops, problems as P  # noqa: E402
from learnmultigrid_amd.solvers import CG, GMRES  # noqa: E402

DEV = "cuda:0"
REPS = 5
TARGET = 1e-8
MAX_ITERATIONS = 600
SMOOTH = dict(precond_steps=2, precond_omega=0.5)


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


def solve(solver, A, b, H, **kw):
    """(iterations, seconds, final residual / ||b||) of one preconditioned Krylov solve, the median of 3."""
    nb = float(np.linalg.norm(b))
    s = solver(A, b.reshape(-1, 1).copy())
    its = []

    def run():
        before = s.get_iterations()                       # (CG counts on from solve to solve, as the reference does)
        s.solve(max_iterations=MAX_ITERATIONS, error=TARGET * nb, preconditioner=H, **SMOOTH, **kw)
        its.append(s.get_iterations() - before if solver is CG else s.get_iterations())

    t, _ = timed(run, reps=3)
    return its[-1], round(t, 4), float(s.get_residual() / nb)


def device(m):
    A, b, B, _ = P.elasticity_2d(m)
    b = np.asarray(b, dtype=np.float64).ravel()
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    n = dA.shape[0]
    X = torch.from_numpy(B).to(DEV)
    t_c, C = timed(lambda: agn.condense_device(dA, 2))
    t_s, S = timed(lambda: agn.symmetric_strength_device(C, 0.0))
    t_a, (agg, n_agg, rounds) = timed(lambda: agn.aggregate_device(S))
    t_t, (T, Bc) = timed(lambda: agn.tentative_block_device(agg, n_agg, 2, X))
    t_p, P1 = timed(lambda: agn.smooth_prolongator_device(dA, T, 4.0 / 3.0))
    t_level, _ = timed(lambda: agn.transfer_device(dA, X, block_size=2))
    out = {"elements_per_side": m, "unknowns": n, "nnz": dA.nnz, "reps": REPS,
           "condense_s": round(t_c, 5), "strength_s": round(t_s, 5), "aggregate_s": round(t_a, 5), "mis2_rounds": rounds,
           "n_agg": n_agg, "tentative_k3_s": round(t_t, 5), "jacobi_step_s": round(t_p, 5), "one_level_s": round(t_level, 5),
           "T_nnz": T.nnz, "P_nnz": P1.nnz}
    del C, S, agg, T, Bc, P1
    setups = (("rigid_body_modes", dict(B=X, block_size=2)), ("translations", dict(block_size=2)), ("ones", dict()))
    for name, kw in setups:
        t_all, H = timed(lambda: agn.sa_hierarchy(dA, DEV, **kw), reps=3)
        info = agn.hierarchy_info(H)
        cg = solve(CG, A, b, H)
        fg = solve(GMRES, A, b, H, restart=20, precond_cycle_shape="K", precond_k_inner="fcg")
        out[name] = {"hierarchy_s": round(t_all, 4), "level_sizes": H.sizes,
                     "operator_complexity": round(info["operator_complexity"], 3),
                     "grid_complexity": round(info["grid_complexity"], 3),
                     "cg_v22_iterations": cg[0], "cg_v22_s": cg[1], "cg_v22_residual": cg[2],
                     "gmres_k_iterations": fg[0], "gmres_k_s": fg[1], "gmres_k_residual": fg[2],
                     "setup_plus_cg_s": round(t_all + cg[1], 4)}
        print("# %d %s %s" % (m, name, json.dumps(out[name])), file=sys.stderr, flush=True)
        del H
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    del dA
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for m in [int(a) for a in sys.argv[1:]] or [1024, 2048]:
        device(m)
