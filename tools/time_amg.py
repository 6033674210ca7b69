#!/usr/bin/env python3
"""Time the stages of the classical AMG setup (learnmultigrid_amd/amg.py, csrc/amg.hip) on an MI355X: on
jittered_poisson_2d(m) -- (m + 1)^2 nodes -- the strength pattern, the PMIS split (with its rounds), direct interpolation,
the Jacobi step on P (its SpGEMM A P apart from the merge), all of one level, and the whole classical_hierarchy down to
max_coarse = 500 with its level sizes and complexities.  Each stage is warmed once; the figure is the median of REPS runs,
host clock around a device synchronise.  One JSON line per size.  Then the plain-Python twin of the rules
(tests/amg_ref.py) on one level of a small problem, host clock: the line that says what "no care for speed" means.

It promises no number: whoever runs it writes the figures and the date into DESIGN.md and README.md.

Usage:  python tools/time_amg.py [--twin M] [elements per side ...]      (default 1024 2048: 1025^2 and 2049^2 nodes; twin 256)"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from learnmultigrid_amd import amg, ops, problems as P  # noqa: E402

DEV = "cuda:0"
REPS = 5


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


def device(m):
    A, _ = P.jittered_poisson_2d(m)
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    t_s, S = timed(lambda: amg.strength_device(dA, 0.25))
    t_split, (state, rank, n_c, rounds) = timed(lambda: amg.pmis_device(S))
    t_direct, P0 = timed(lambda: amg.direct_interpolation_device(dA, S, state, rank, n_c))
    t_ap, AP = timed(lambda: ops.spgemm(dA, P0))
    t_merge, P1 = timed(lambda: ops.amg_smooth(dA, P0, AP, state, rank, 1.0, 0.2))
    t_level, _ = timed(lambda: amg.transfer_device(dA))
    t_all, H = timed(lambda: amg.classical_hierarchy(dA, DEV), reps=3)
    info = amg.hierarchy_info(H)
    print(json.dumps({
        "elements_per_side": m, "nodes": dA.shape[0], "nnz": dA.nnz, "reps": REPS,
        "strength_s": round(t_s, 5), "pmis_s": round(t_split, 5), "pmis_rounds": rounds, "n_c": n_c,
        "direct_s": round(t_direct, 5), "spgemm_AP_s": round(t_ap, 5), "jacobi_merge_s": round(t_merge, 5),
        "one_level_s": round(t_level, 5), "P_nnz_direct": P0.nnz, "P_nnz_smoothed": P1.nnz,
        "hierarchy_s": round(t_all, 4), "level_sizes": H.sizes,
        "operator_complexity": round(info["operator_complexity"], 3), "grid_complexity": round(info["grid_complexity"], 3)}),
        flush=True)
    del H, dA, S, P0, P1, AP
    torch.cuda.empty_cache()


def twin(m):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import amg_ref as R
    A, _ = P.jittered_poisson_2d(m)
    t0 = time.perf_counter()
    Pm, info = R.transfer(A)
    print(json.dumps({"twin_elements_per_side": m, "nodes": A.shape[0], "one_level_s": round(time.perf_counter() - t0, 3),
                      "n_c": info["n_c"], "pmis_rounds": info["rounds"], "P_nnz_smoothed": int(Pm.nnz)}), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    twin_m = 256
    if "--twin" in args:
        k = args.index("--twin")
        twin_m = int(args[k + 1])
        del args[k:k + 2]
    for m in [int(a) for a in args] or [1024, 2048]:
        device(m)
    twin(twin_m)
