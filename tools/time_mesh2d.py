#!/usr/bin/env python3
"""Time the first stage of the 2-D workflow on an MI355X: mesh.Mesh2D(k * k) -> refine(True) -> p1(), three figures:
the refinement (edge keys, sort, runs, scan, nodes and children), the device topology (P1Mesh2D.from_device: sort,
search, adjacency, pattern count / scan / fill), and, in the same process on the same downloaded (p, conn), the host
constructor P1Mesh2D.__init__ with its uploads.  Each stage is warmed once; the figure is the median of REPS runs, host
clock around a device synchronise.  The two topologies are compared integer for integer.  One JSON line per size.

Usage:  python tools/time_mesh2d.py [squares per side before refinement ...]      (default 1024: 2049^2 nodes)"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learnmultigrid_amd import Mesh2D  # noqa: E402
from learnmultigrid_amd.assembly import P1Mesh2D  # noqa: E402

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
    return statistics.median(ts), min(ts), max(ts), out


def main(sides):
    for k in sides:
        t_con, _, _, coarse = timed(lambda: Mesh2D(k * k, device=DEV))
        px, py, conn = coarse.px, coarse.py, coarse.dconn

        def refine():
            m = Mesh2D.__new__(Mesh2D)                    # the same unrefined arrays every time
            m.device, m.px, m.py, m.dconn = coarse.device, px, py, conn
            m._p = m._conn = m._boundary = m._p1 = None
            return m.refine(True)
        t_ref, ref_lo, ref_hi, fine = timed(refine)
        t_top, top_lo, top_hi, dev = timed(lambda: P1Mesh2D.from_device(fine.px, fine.py, fine.dconn, checked=True))
        t_bnd, _, _, _ = timed(lambda: (setattr(fine, "_boundary", None), fine.boundary_nodes()))
        p, c = fine.p, fine.conn
        t_host, host_lo, host_hi, host = timed(lambda: P1Mesh2D(p, c, DEV))
        same = all(torch.equal(getattr(dev, a), getattr(host, a))
                   for a in ("n2e_ptr", "n2e_elem", "n2e_loc", "rowptr", "colidx"))
        print(json.dumps({
            "squares_per_side": k, "nodes": fine.n_p, "elements": fine.ne, "nnz": dev.nnz, "reps": REPS,
            "construct_s": round(t_con, 5),
            "refine_s": round(t_ref, 5), "refine_min_max_s": [round(ref_lo, 5), round(ref_hi, 5)],
            "device_topology_s": round(t_top, 5), "device_topology_min_max_s": [round(top_lo, 5), round(top_hi, 5)],
            "boundary_nodes_s": round(t_bnd, 5),
            "host_topology_s": round(t_host, 4), "host_topology_min_max_s": [round(host_lo, 4), round(host_hi, 4)],
            "host_over_device": round(t_host / t_top, 1), "same_integers": bool(same)}), flush=True)
        del coarse, fine, dev, host
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [1024])
