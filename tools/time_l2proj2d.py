#!/usr/bin/env python3
"""Time l2_projection.transfer_2d_device("pseudo", ...) on an MI355X: a jittered (m+1)^2 mesh over its every-second-node
coarse mesh (problems.jittered_mesh_2d / coarsen_mesh_2d), split into the candidate search (cell grid, sort, candidate
lists) and the rows (count, scan, fill), each synchronised; and the host twin (transfer_2d) at 257^2 fine nodes in the
same run.  Preparing a P1Mesh2D (host integer work, once per mesh) is reported but not part of the transfer.  One JSON
line per size.

Usage:  python tools/time_l2proj2d.py [fine nodes per side ...]"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learnmultigrid_amd import l2_projection as L2, problems as P  # noqa: E402
from learnmultigrid_amd.assembly import P1Mesh2D  # noqa: E402

DEV = "cuda:0"
HOST_SIDE = 257


def timed(f, reps=3):
    best, out = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def main(sides):
    for side in sides:
        m = side - 1
        pf, cf = P.jittered_mesh_2d(m)
        pc, cc = P.coarsen_mesh_2d(pf, m)
        t0 = time.perf_counter()
        fine, coarse = P1Mesh2D(pf, cf, DEV), P1Mesh2D(pc, cc, DEV)
        prep = time.perf_counter() - t0
        L2.transfer_2d_device("pseudo", fine, coarse)                                   # warm: code objects, allocator
        t_search, (candptr, cand) = timed(lambda: L2.candidates_2d_device(fine, coarse))
        t_rows, Q = timed(lambda: L2.rows_2d_device(1, fine, coarse, candptr, cand))
        t_all, _ = timed(lambda: L2.transfer_2d_device("pseudo", fine, coarse))
        row = {"fine_nodes": fine.n, "coarse_nodes": coarse.n, "fine_elements": fine.ne, "pairs": int(cand.numel()),
               "nnz": Q.nnz, "mesh_prepare_s": round(prep, 3), "search_s": round(t_search, 5), "rows_s": round(t_rows, 5),
               "transfer_s": round(t_all, 5), "ns_per_pair_rows": round(1e9 * t_rows / max(1, cand.numel()), 2)}
        if side == HOST_SIDE:
            t0 = time.perf_counter()
            T = L2.transfer_2d("pseudo", pf, cf, pc, cc)
            row["host_twin_s"] = round(time.perf_counter() - t0, 3)
            D = Q.to_scipy() - T
            row["max_abs_diff_to_twin"] = float(abs(D).max())
        print(json.dumps(row), flush=True)
        del fine, coarse, candptr, cand, Q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [HOST_SIDE, 1025, 2049])
