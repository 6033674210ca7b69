#!/usr/bin/env python3
"""Time the Chebyshev smoother against weighted Jacobi (the numbers of DESIGN.md section 3, "Chebyshev polynomial smoother"):
  passes    tiled Chebyshev pass vs tiled Jacobi pass vs the two-launch path (residual + lmg_cheby_update per sweep), the
            four forms, 1 - 3 sweeps, each a hipGraph chain of --chain launches replayed --reps times; the Jacobi pass is
            measured twice (before and after the others): the spread between the two is the run's noise
  cycle     cfg#4 V(3,3) cycle time, Chebyshev and Jacobi(0.8), hipGraph replay, and the cycles either needs to 1e-10
    python tools/time_cheby.py passes --size 1024 [--level 0] [--kind 5pt|9pt]
    python tools/time_cheby.py cycle [--size 4096 --levels 6]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from learnmultigrid_amd import ops, problems as P
from learnmultigrid_amd.hierarchy import Hierarchy, chebyshev_coefficients

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["passes", "cycle"])
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--levels", type=int, default=0)
ap.add_argument("--level", type=int, default=0)
ap.add_argument("--chain", type=int, default=20)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--sweeps", default="1,2,3")
a = ap.parse_args()
dev = torch.device("cuda:0")
m = a.size
A, rhs = P.poisson_2d_structured(m)
levels = a.levels or (6 if m >= 2048 else 4)
H = Hierarchy(A, P.geometric_hierarchy_2d(m + 1, levels), dev)


def chain_time(f):
    """us per call of f inside a hipGraph chain."""
    with torch.cuda.stream(H.stream):
        f()
        g = ops.CapturedGraph()
        with g:
            for _ in range(a.chain):
                f()
        for _ in range(2):
            g.launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            g.launch()
        e1.record()
        e1.synchronize()
    return e0.elapsed_time(e1) / (a.reps * a.chain) * 1e3


if a.what == "passes":
    lev = H.levels[a.level]
    fa = lev.A
    n, nc = fa.shape[0], lev.P.shape[1]
    print("level %d of %d^2: n = %d, Jacobi pass %s, Chebyshev pass %s" % (a.level, m + 1, n, ops._fused_kind(fa), ops._cheby_kind(fa)))
    with torch.cuda.stream(H.stream):
        x = torch.rand(n, dtype=torch.float64, device=dev); b = torch.rand_like(x); y = torch.empty_like(x); r = torch.empty_like(x)
        e = torch.rand(nc, dtype=torch.float64, device=dev); bc = torch.empty_like(e)
        d = torch.zeros_like(x); dinv = ops.csr_inverse_diagonal(fa)
    tiled_jacobi = ops._fused_kind(fa) == "tile"
    for S in [int(s) for s in a.sweeps.split(",")]:
        coef = chebyshev_coefficients(2.0, 4.0, S)

        def two_launch():
            for k, (ca, cc) in enumerate(coef):
                ops.csr_residual_norm2(fa, x, b, r, None, None)
                ops.cheby_update(ca, cc, dinv, r, d, x, first=(k == 0))

        def two_launch_resid():
            two_launch()
            ops.csr_residual_norm2(fa, x, b, r, None, None)

        jac = {"plain": lambda: ops.stencil_smooth(fa, x, b, 0.8, S, y, None),
               "resid": lambda: ops.stencil_smooth(fa, x, b, 0.8, S, y, r),
               "zero": lambda: ops.stencil_smooth(fa, None, b, 0.8, S, y, None),
               "prol": lambda: ops.stencil_smooth(fa, x, b, 0.8, S, y, None, prolong=(lev.P, e)),
               "rest": lambda: ops.stencil_smooth(fa, x, b, 0.8, S, y, None, restrict=(lev.R, bc))}
        che = {"plain": lambda: ops.stencil_cheby(fa, x, b, coef, y, None),
               "resid": lambda: ops.stencil_cheby(fa, x, b, coef, y, r),
               "zero": lambda: ops.stencil_cheby(fa, None, b, coef, y, None),
               "prol": lambda: ops.stencil_cheby(fa, x, b, coef, y, None, prolong=(lev.P, e)),
               "rest": lambda: ops.stencil_cheby(fa, x, b, coef, y, None, restrict=(lev.R, bc))}
        for form in ("plain", "resid", "zero", "prol", "rest"):
            j1 = chain_time(jac[form]) if tiled_jacobi or form in ("plain", "resid", "zero") else float("nan")
            c = chain_time(che[form])
            j2 = chain_time(jac[form]) if j1 == j1 else j1
            print("S=%d %-5s  Jacobi pass %.2f / %.2f us   Chebyshev pass %.2f us   (+%.1f %% over the Jacobi mean)"
                  % (S, form, j1, j2, c, 100 * (c / ((j1 + j2) / 2) - 1)), flush=True)
        print("S=%d two-launch path: plain %.2f us, + residual %.2f us" % (S, chain_time(two_launch), chain_time(two_launch_resid)), flush=True)
else:
    import math
    fine = H.levels[0]
    with torch.cuda.stream(H.stream):
        fine.b.copy_(torch.from_numpy(rhs.ravel().copy()).to(dev))
        for sm, om in (("Jacobi", 0.8), ("Chebyshev", 1.0), ("Jacobi", 0.8), ("Chebyshev", 1.0)):
            g = H.captured_cycle(sm, 3, om, "lexicographic")
            ops.zero(fine.x)
            for _ in range(3):
                g.launch()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                g.launch()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            ops.zero(fine.x)
            r0 = H.residual_norm()
            its = 0
            while H.residual_norm(False) > 1e-10 and its < 60:
                g.launch()
                its += 1
            print("%d^2, %d levels, V(3,3) %-9s %.4f ms per cycle; %d cycles to ||r|| <= 1e-10 (from %.3e); kinds %s"
                  % (m + 1, levels, sm, ms, its, r0,
                     [ops._cheby_kind(l.A) if sm == "Chebyshev" else ops._fused_kind(l.A) for l in H.levels[:-1]]), flush=True)
