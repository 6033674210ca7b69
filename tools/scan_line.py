#!/usr/bin/env python3
"""Time the line relaxation kernels on the 5-point anisotropic operator (ax = 1e-3, ay = 1) next to the point smoothers'
kernels, and the time to ||r|| <= 1e-8 of the cycles built on them.   python tools/scan_line.py [--sizes 1024,2048,4096]
[--solve-size 2048] [--reps 30]     (one process, HIP events, warm-up; sizes are elements per side: 1024 -> 1025^2 nodes)"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from learnmultigrid_amd import ops, problems as P
from learnmultigrid_amd.hierarchy import Hierarchy

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1024,2048,4096")
ap.add_argument("--solve-size", type=int, default=2048)
ap.add_argument("--levels", type=int, default=6)
ap.add_argument("--reps", type=int, default=30)
a = ap.parse_args()
dev = torch.device("cuda:0")


def timeit(f, reps):
    for _ in range(3): f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for m in [int(s) for s in a.sizes.split(",") if s]:
    A, _ = P.anisotropic_poisson_2d_structured(m, 1e-3, 1.0)
    dA = ops.DeviceCSR.from_scipy(A, dev)
    dA.pack()
    W, n = m + 1, (m + 1) ** 2
    fac = {d: ops.line_factor(dA, W, d) for d in "xy"}
    x = torch.rand(n, dtype=torch.float64, device=dev); b = torch.rand_like(x); r = torch.empty_like(x); y = torch.empty_like(x)

    def step():
        for d in "xy":
            for first in (0, 1):
                ops.csr_residual_norm2(dA, x, b, r, None, None)
                ops.line_solve(W, d, first, 2, fac[d], r, 1.0, x)

    calls = {"residual": lambda: ops.csr_residual_norm2(dA, x, b, r, None, None)}
    for d in "xy":
        calls["solve %s all" % d] = lambda d=d: ops.line_solve(W, d, 0, 1, fac[d], r, 1.0, x)
        calls["solve %s one colour" % d] = lambda d=d: ops.line_solve(W, d, 0, 2, fac[d], r, 1.0, x)
    calls["xy zebra step (4 residuals + 4 solves)"] = step
    calls["stencil_smooth, 1 sweep"] = lambda: ops.stencil_smooth(dA, x, b, 0.8, 1, y)
    if ops.stencil_gs_available(dA):
        calls["stencil_gs, 1 sweep"] = lambda: ops.stencil_gs(dA, x, b, 1)
    print("%d^2 (n = %d, %d waves of systems per direction):" % (W, n, (W + 63) // 64))
    for k, f in calls.items():
        x.uniform_(); r.uniform_()                      # (the solves feed on their own output: keep the numbers finite)
        print("    %-42s %9.1f us" % (k, timeit(f, a.reps)), flush=True)
    del dA, fac, x, b, r, y

m = a.solve_size
if m > 0:
    A, rhs = P.anisotropic_poisson_2d_structured(m, 1e-3, 1.0)
    H = Hierarchy(A, P.geometric_hierarchy_2d(m + 1, a.levels), dev)
    fine = H.levels[0]
    print("time to ||r|| <= 1e-8 at %d^2, %d levels, ax = 1e-3 (eager launches, one norm read per cycle):" % (m + 1, a.levels))
    with torch.cuda.stream(H.stream):
        for name, args, kw, cap in (("Line xy zebra V(1,1)", ("Line", 1, 1.0), dict(line_dir="xy", line_order="zebra"), 200),
                                    ("Line y zebra V(1,1)", ("Line", 1, 1.0), dict(line_dir="y", line_order="zebra"), 200),
                                    ("Jacobi 0.8 V(3,3)", ("Jacobi", 3, 0.8), {}, 200),
                                    ("Chebyshev degree 3", ("Chebyshev", 3, 1.0), {}, 200)):
            H.prepare_smoother(args[0], **kw)
            for timed in (False, True):                 # the first pass warms every kernel and twin up
                fine.b.copy_(torch.from_numpy(rhs.ravel().copy()).to(dev))
                ops.zero(fine.x)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cycles, res = 0, H.residual_norm()
                while res > 1e-8 and cycles < cap:
                    H.cycle(*args)
                    cycles += 1
                    res = H.residual_norm()
                torch.cuda.synchronize()
                t = time.perf_counter() - t0
            print("    %-24s %4d cycles%s  %9.2f ms   ||r|| = %.2e" % (name, cycles, " (cap)" if res > 1e-8 else "      ", t * 1e3, res),
                  flush=True)
