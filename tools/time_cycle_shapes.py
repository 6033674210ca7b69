#!/usr/bin/env python3
"""V-, W- and F-cycles with and without the turnaround pass, in one process: cfg#2 (513^2, 3 levels) and cfg#4
(4097^2, 6 levels), weighted Jacobi (omega = 0.8) with `--nu` sweeps on either side.  Every cycle is captured into a
hipGraph once per setting and the replays are timed round-robin.  Then, on every level of cfg#4 that runs the tiled
passes, the turnaround pass (lmg_stencil_smooth_tiled_turnaround) against the correcting pass followed by the
restricting pass it replaces, each captured `--reps` times into one graph, for 32- and 64-line turnaround tiles.

  python tools/time_cycle_shapes.py [--nu 3] [--rounds 5] [--steps 20] [--reps 50]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from learnmultigrid_amd import ops, problems as P  # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nu", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--configs", default="cfg2,cfg4")
ap.add_argument("--no-levels", action="store_true", help="skip the per-level pass timings")
a = ap.parse_args()
CONFIGS = {"cfg2": (512, 3), "cfg4": (4096, 6)}
dev = torch.device("cuda:0")


def timed(fn, steps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def med(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def cycles(name, m, levels):
    A, rhs = P.poisson_2d_structured(m)
    H = Hierarchy(A, P.geometric_hierarchy_2d(m + 1, levels), dev)
    H.levels[0].b.copy_(torch.from_numpy(rhs.ravel().copy()).to(dev))
    H.stream.wait_stream(torch.cuda.current_stream())
    settings = [(s, t) for s in "VWF" for t in (True, False) if not (s == "V" and not t)]
    graphs = {}
    with torch.cuda.stream(H.stream):
        for shape, turn in settings:
            ops.set_fused_turnaround_enabled(turn)
            H._graphs.clear()
            graphs[(shape, turn)] = H.captured_cycle("Jacobi", a.nu, 0.8, "lexicographic", shape=shape)
        ops.set_fused_turnaround_enabled(True)
        times = {k: [] for k in settings}
        for _ in range(a.rounds):
            for k in settings:
                times[k].append(timed(graphs[k].launch, a.steps))
    print("%s (%d^2, %d levels), %s(%d,%d) Jacobi, hipGraph replay" % (name, m + 1, levels, "cycle", a.nu, a.nu))
    for (shape, turn), t in times.items():
        md, lo, hi = med(t)
        print("  %s-cycle  turnaround %-3s  median %.4f ms   min %.4f   max %.4f"
              % (shape, "on" if turn else "off", md, lo, hi))
    return H


def levels(H):
    print("per level, %d + %d sweeps: turnaround pass vs correcting + restricting pass (us per pair, graph of %d)"
          % (a.nu, a.nu, a.reps))
    for l, lev in enumerate(H.levels[:-1]):
        if not ops.stencil_smooth_turnaround_available(lev.A, lev.P, lev.R):
            continue
        nxt = H.levels[l + 1]
        n = lev.n
        x = torch.randn(n, dtype=torch.float64, device=dev)
        y, z = torch.empty_like(x), torch.empty_like(x)
        e = torch.randn(nxt.n, dtype=torch.float64, device=dev)
        bc = torch.empty_like(e)
        b = lev.b

        def two():
            ops.stencil_smooth(lev.A, x, b, 0.8, a.nu, y, None, prolong=(lev.P, e))
            ops.stencil_smooth(lev.A, y, b, 0.8, a.nu, z, None, restrict=(lev.R, bc))

        def one():
            ops.stencil_smooth_turnaround(lev.A, x, b, 0.8, a.nu, a.nu, z, prolong=(lev.P, e), restrict=(lev.R, bc))

        res = {}
        with torch.cuda.stream(H.stream):
            for key, fn, rows in (("two", two, None), ("one32", one, 32), ("one64", one, 64)):
                if rows is not None:
                    ops.tune_set("tile_turnaround_rows", rows)
                g = ops.CapturedGraph()
                with g:
                    for _ in range(a.reps):
                        fn()
                ops.tune_set("tile_turnaround_rows", 0)
                res[key] = g
            t = {k: [] for k in res}
            for _ in range(a.rounds):
                for k, g in res.items():
                    t[k].append(timed(g.launch, 3) * 1e3 / a.reps)
        side = int(round(n ** 0.5))
        print("  level %d  %d^2  two passes %.1f us   turnaround 32-line %.1f us   64-line %.1f us"
              % (l, side, med(t["two"])[0], med(t["one32"])[0], med(t["one64"])[0]))


for cfg in a.configs.split(","):
    m, lv = CONFIGS[cfg]
    H = cycles(cfg, m, lv)
    if cfg == "cfg4" and not a.no_levels:
        levels(H)
    del H
    torch.cuda.empty_cache()
