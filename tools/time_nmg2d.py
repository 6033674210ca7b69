#!/usr/bin/env python3
"""Time NeuralMG_2D.define_hierarchy(levels=3) on an MI355X: P1 mass matrices of structured triangulations with 257^2 and
1025^2 nodes, an element-wise stand-in model (NumPy on the host, like any caller's model), and the split over the stages
(seconds, summed over the two levels; every stage is synchronised for it, so the sum is an upper bound of an untimed run,
which is reported too).  One JSON line per size.

Usage:  python tools/time_nmg2d.py [nodes per side ...]"""
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learnmultigrid_amd.solvers import NeuralMG_2D  # noqa: E402


class ElementwiseModel:
    def predict(self, data):
        return 0.25 + 0.125 * np.abs(np.sin(1e3 * data[:, :31] + np.arange(31.0)))


def p1_mass(m):
    """P1 mass matrix of the m x m structured triangulation of the unit square, cells cut along one diagonal."""
    h = 1.0 / (m - 1)
    i, j = np.meshgrid(np.arange(m - 1), np.arange(m - 1), indexing="ij")
    a = (j * m + i).ravel()
    tris = np.concatenate([np.stack([a, a + 1, a + m + 1], 1), np.stack([a, a + m + 1, a + m], 1)])
    loc = h * h / 24.0 * (np.ones((3, 3)) + np.eye(3))
    rows, cols = np.repeat(tris, 3, axis=1).ravel(), np.tile(tris, (1, 3)).ravel()
    return sp.coo_matrix((np.tile(loc.ravel(), len(tris)), (rows, cols)), shape=(m * m, m * m)).tocsr()


def main(sides):
    for m in sides:
        M = p1_mass(m)
        n = M.shape[0]
        nmg = NeuralMG_2D(sp.identity(n, format="csr"), np.ones((n, 1)), ElementwiseModel(), M, np.ones(43), np.zeros(43))
        nmg.define_hierarchy(levels=3)                      # warm: code objects, allocator
        t0 = time.perf_counter()
        nmg.define_hierarchy(levels=3)
        plain = time.perf_counter() - t0
        nmg.define_hierarchy(levels=3, timed=True)
        print(json.dumps({"nodes": n, "levels": 3, "sizes": [n] + [Q.shape[1] for Q in nmg.l_hierarchy],
                          "define_hierarchy_s": round(plain, 4),
                          "stages_s": {k: round(v, 4) for k, v in nmg.setup_timings.items()}}), flush=True)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [257, 1025])
