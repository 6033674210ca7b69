#!/usr/bin/env python3
"""Time multicolour Gauss-Seidel with its setup on the device (gs_mode="multicolor_device": ops.color_device,
ops.build_gs_schedule_device, csrc/color.hip) on an MI355X, level by level on the classical AMG hierarchy of
jittered_poisson_2d(m) -- (m + 1)^2 nodes --, next to what the same level costs on the paths that were there before:

  per level   colouring (with its rounds and colours), the colour-ordered sliced-ELL twin, one sweep of the new kernel;
              the host colouring of gs_mode="multicolor" with its device-to-host copy of the pattern, one sweep of that
              schedule through ops.csr_gs_schedule, one sweep of the device-built schedule through the same executors (what a
              level below the crossover would run), and one damped-Jacobi sweep of the level's own twin -- the bandwidth yardstick;
  per size    GMRES(10) preconditioned with V(2,2) to 1e-8 ||b||: damped Jacobi (0.8) against Gauss-Seidel in the new mode.

Each stage is warmed once; the figure is the median of REPS runs, host clock around a device synchronise.  One JSON line per
level and one per size.  It promises no number: whoever runs it writes the figures and the date into DESIGN.md and README.md.

Usage:  python tools/time_color_gs.py [elements per side ...]      (default 1024 2048: 1025^2 and 2049^2 nodes)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from learnmultigrid_amd import amg, ops, problems as P, smoothing  # noqa: E402
from learnmultigrid_amd.solvers import GMRES  # noqa: E402

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


def level(m, l, A):
    n = A.shape[0]
    x = torch.zeros(n, dtype=torch.float64, device=DEV)
    y = torch.zeros_like(x)
    b = torch.ones_like(x)
    t_color, (color, nc, rounds) = timed(lambda: ops.color_device(A))
    t_all, sched = timed(lambda: ops.build_gs_schedule_device(A))
    t_twin, _ = timed(lambda: ops.ColorSell.from_schedule(A, sched.d_rows, sched.h_ptr))
    t_sweep, _ = timed(lambda: ops.csr_gs_schedule(A, x, b, sched, 1))

    def host_setup():
        return smoothing.gs_schedule(ops, A, A.rowptr.cpu().numpy(), A.colidx.cpu().numpy(), "multicolor", DEV)

    t_host, hsched = timed(host_setup, reps=3)
    t_host_sweep, _ = timed(lambda: ops.csr_gs_schedule(A, x, b, hsched, 1))
    plain = ops.GSSchedule("multicolor", sched.d_rows.cpu().numpy(), sched.h_ptr, DEV)
    ops.gs_prepare(A, plain)
    t_plain_sweep, _ = timed(lambda: ops.csr_gs_schedule(A, x, b, plain, 1))
    t_jacobi, _ = timed(lambda: ops.csr_jacobi(A, x, b, 0.8, y))
    sizes = np.diff(sched.h_ptr)
    print(json.dumps({
        "elements_per_side": m, "level": l, "n": n, "nnz": A.nnz, "longest_row": sched.twin.max_len,
        "colours": nc, "rounds": rounds, "smallest_colour": int(sizes.min()), "largest_colour": int(sizes.max()),
        "padded_over_nnz": round(sched.twin.padded / max(A.nnz, 1), 3),
        "colour_s": round(t_color, 6), "twin_s": round(t_twin, 6), "setup_s": round(t_all, 6), "sweep_s": round(t_sweep, 7),
        "host_multicolor_setup_s": round(t_host, 6), "host_multicolor_colours": hsched.nsets,
        "host_multicolor_sweep_s": round(t_host_sweep, 7), "csr_sweep_on_device_schedule_s": round(t_plain_sweep, 7),
        "jacobi_sweep_s": round(t_jacobi, 7)}), flush=True)


def solve(m, A, rhs, H):
    nb = float(np.linalg.norm(rhs))
    out = {"elements_per_side": m, "levels": H.sizes}
    for name, kw in (("jacobi", dict(precond_smoother="Jacobi", precond_omega=0.8)),
                     ("multicolor_device", dict(precond_smoother="GaussSeidel", precond_gs_mode="multicolor_device"))):
        g = GMRES(A, rhs.reshape(-1, 1).copy())
        t, _ = timed(lambda: g.solve(max_iterations=200, error=1e-8 * nb, restart=10, preconditioner=H, precond_steps=2, **kw),
                     reps=3)                              # (the warming run also builds the schedules and twins of the mode)
        out["gmres10_%s_s" % name] = round(t, 5)
        out["gmres10_%s_iterations" % name] = g.get_iterations()
        out["gmres10_%s_converged" % name] = bool(g.get_residual() <= 1e-8 * nb)
    print(json.dumps(out), flush=True)


def device(m):
    A, rhs = P.jittered_poisson_2d(m)
    t_h, H = timed(lambda: amg.classical_hierarchy(A, DEV), reps=1)
    print(json.dumps({"elements_per_side": m, "hierarchy_s": round(t_h, 4), "level_sizes": H.sizes}), flush=True)
    for l, lev in enumerate(H.levels[:-1]):
        try:
            level(m, l, lev.A)
        except ops.LmgError as e:                         # (a level that needs more than 64 colours: said, not hidden)
            print(json.dumps({"elements_per_side": m, "level": l, "n": lev.n, "refused": str(e)}), flush=True)
    try:
        solve(m, A, np.asarray(rhs, dtype=np.float64).ravel(), H)
    except ops.LmgError as e:
        print(json.dumps({"elements_per_side": m, "solve_refused": str(e)}), flush=True)
    del H
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for m in [int(a) for a in sys.argv[1:]] or [1024, 2048]:
        device(m)
