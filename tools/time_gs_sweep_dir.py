#!/usr/bin/env python3
"""Forward against backward exact Gauss-Seidel, in one process (gs_wave.hip, lmg_stencil_gs_sweep[_backward]):

  * 3-sweep launches (one pipelined MULTI launch each) at 4097^2 (5-point) and 2049^2 (9-point Galerkin R A P of cfg#4),
    forward and backward alternating, HIP events around each launch, median of --reps;
  * the cfg#4 V(3,3) cycle (hipGraph replay) with forward Gauss-Seidel on both sides (the reference's shipped smoother)
    against forward pre- / backward post-smoothing;
  * MG-PCG (cfg#4 hierarchy, symmetric interior-block variant of the 4097^2 operator) to ||r|| <= 1e-10 with the
    weighted-Jacobi V(2,2) preconditioner and with the ("forward", "backward") Gauss-Seidel V(2,2) one.

  python3 tools/time_gs_sweep_dir.py [--reps 15] [--no-pcg]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                           # noqa: E402
import scipy.sparse as sp                                    # noqa: E402
import torch                                                 # noqa: E402

from learnmultigrid_amd import ops, problems as P            # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy           # noqa: E402

DEV = "cuda:0"


def sweep_times(A, reps, label):
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack()
    assert ops.stencil_gs_available(dA, "backward"), label
    n = A.shape[0]
    g = torch.Generator().manual_seed(1)
    x = torch.rand(n, dtype=torch.float64, generator=g).to(DEV)
    b = torch.rand(n, dtype=torch.float64, generator=g).to(DEV)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {"forward": [], "backward": []}
    for k in range(reps + 2):
        for d in ("forward", "backward") if k % 2 == 0 else ("backward", "forward"):
            ev[0].record()
            ops.stencil_gs(dA, x, b, 3, d)
            ev[1].record()
            ev[1].synchronize()
            if k >= 2:
                t[d].append(ev[0].elapsed_time(ev[1]))
    ops.stencil_gs_check(dA)
    f, bw = np.median(t["forward"]), np.median(t["backward"])
    print("%-34s 3 sweeps, one launch: forward %.3f ms (min %.3f), backward %.3f ms (min %.3f), backward / forward %.3f"
          % (label, f, min(t["forward"]), bw, min(t["backward"]), bw / f), flush=True)


def cycle_times(A, rhs, hier, reps):
    H = Hierarchy(A, hier, torch.device(DEV))
    H.levels[0].b.copy_(torch.from_numpy(rhs.ravel().copy()).to(DEV))
    H.stream.wait_stream(torch.cuda.current_stream())
    out = {}
    with torch.cuda.stream(H.stream):
        for pair in (("forward", "forward"), ("forward", "backward")):
            g = H.captured_cycle("GaussSeidel", 3, 1.0, "lexicographic", pair)
            for _ in range(2):
                g.launch()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                g.launch()
            torch.cuda.synchronize()
            out[pair] = (time.perf_counter() - t0) / reps * 1e3
        H.check_smoothers()
    for pair, ms in out.items():
        print("cfg#4 V(3,3) cycle, Gauss-Seidel %-22s %.2f ms per cycle (hipGraph replay)" % ("(%s, %s):" % pair, ms), flush=True)


def pcg_times(A, hier):
    from learnmultigrid_amd.solvers import CG
    s = int(round(np.sqrt(A.shape[0])))
    idx = np.arange(s * s)
    inter = ((idx % s) > 0) & ((idx % s) < s - 1) & ((idx // s) > 0) & ((idx // s) < s - 1)
    keep = sp.diags(inter.astype(float))
    As = sp.csr_matrix(keep @ A @ keep + sp.diags((~inter).astype(float)))
    rhs = np.ones(As.shape[0])
    H = Hierarchy(As, hier, torch.device(DEV))
    for sm in ("Jacobi", "GaussSeidel"):
        c = CG(As, rhs.copy())
        c.solve(max_iterations=3, error=1e-10, preconditioner=H, precond_smoother=sm)          # warm-up
        torch.cuda.synchronize()
        c = CG(As, rhs.copy())
        t0 = time.perf_counter()
        c.solve(max_iterations=500, error=1e-10, preconditioner=H, precond_smoother=sm)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print("MG-PCG cfg#4 (symmetric variant), V(2,2) %-12s %3d iterations to ||r|| = %.2e: %.1f ms"
              % (sm + ":", c.get_iterations(), c.get_track_res()[-1, 0], dt * 1e3), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-pcg", action="store_true")
    a = ap.parse_args()
    A, rhs = P.poisson_2d_structured(4096)
    hier = P.geometric_hierarchy_2d(4097, 6)
    sweep_times(A, a.reps, "4097^2 5-point:")
    Pm = sp.csr_matrix(hier[0])
    A1 = sp.csr_matrix(Pm.T.tocsr() @ A @ Pm)
    A1.sort_indices()
    sweep_times(A1, a.reps, "2049^2 9-point Galerkin (R A P):")
    del A1
    cycle_times(A, rhs, hier, 10)
    if not a.no_pcg:
        pcg_times(A, hier)


if __name__ == "__main__":
    main()
