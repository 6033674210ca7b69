#!/usr/bin/env python3
"""Line relaxation with banded line systems (line_band = 2, 3) against the tridiagonal solve and against damped Jacobi.

(a) One half-step of ops.line_solve_banded for p = 2, 3 and of ops.line_solve on the same grid in the same process, both
    directions, one zebra colour (first 0, step 2) and all systems (first 0, step 1), at --sizes (1025^2, 2049^2).  The
    kernels' time does not depend on the values, so the factors are random numbers of the size of real ones (multipliers
    and upper entries around 0.1, minv around 1): no 49-point matrix of 4 M rows is assembled.  Byte model per element of an
    addressed system (8 B per double): tridiagonal forward r, lo, minv -> d and backward d, cp, x -> x, 64 B; banded
    forward r, p multipliers -> d and backward d, minv, p upper entries, x -> x, (2 p + 6) * 8 = 80 / 96 B.
(b) One V(1,1) Line cycle (line_band = 3) on the stretched problem (a_x = 1e-3 a_y) at --size (1025^2) with learned-like
    transfers, 5 levels (half-bandwidths 1 / 2 / 3 / 3), eager and replayed from a hipGraph, line_dir "y" and "xy"; beside it
    the V(1,1) damped-Jacobi cycle of the same hierarchy.
(c) Cycles and wall-clock to |r| <= 1e-8 |b| from a zero guess, random right-hand side, graph replay, one norm read per
    cycle: Line(line_band = 3) against damped Jacobi (omega = 0.8) on that hierarchy.
HIP events around `inner` calls after a call that is not timed; median and minimum over --reps repetitions, the candidates
interleaved.  One JSON line per measurement.
    python tools/time_line_band.py --part abc --sizes 1024 2048 --size 1024"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, scipy.sparse as sp
from learnmultigrid_amd import ops, problems as P
from learnmultigrid_amd.hierarchy import Hierarchy

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="abc")
ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--levels", type=int, default=5)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--max-cycles", type=int, default=1500)
a = ap.parse_args()
dev = "cuda:0"
F64 = torch.float64
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(run, inner):
    """Milliseconds per call of run(), `inner` calls between two events on the current stream, after one call that is not
    timed."""
    run(); torch.cuda.synchronize()
    ev0.record()
    for _ in range(inner): run()
    ev1.record(); torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / inner


def interleaved(runs, one):
    """{name: times} over a.reps repetitions (one more is dropped), every candidate once per repetition."""
    res = {k: [] for k in runs}
    for rep in range(a.reps + 1):
        for k, run in runs.items():
            t = one(run)
            if rep: res[k].append(t)
    return {k: np.array(v) for k, v in res.items()}


if "a" in a.part:
    for m in a.sizes:
        W = m + 1
        n = W * W
        x, r0, r = (torch.rand(n, dtype=F64, device=dev) for _ in range(3))
        tri = (0.1 * torch.rand(n, dtype=F64, device=dev), 0.5 + 0.5 * torch.rand(n, dtype=F64, device=dev),
               0.1 * torch.rand(n, dtype=F64, device=dev))
        facs = {}
        for p in ops.LINE_SOLVE_BANDS:
            f = 0.1 * torch.rand((2 * p + 1) * n, dtype=F64, device=dev)
            f[p * n:(p + 1) * n] = 0.5 + 0.5 * torch.rand(n, dtype=F64, device=dev)
            facs[p] = f
        for d in "xy":
            for first, step in ((0, 2), (0, 1)):
                def run_tri():
                    ops.copy(r0, r); ops.line_solve(W, d, first, step, tri, r, 1.0, x)

                def run_band(p):
                    return lambda: (ops.copy(r0, r), ops.line_solve_banded(W, d, p, first, step, facs[p], r, 1.0, x))

                runs = {"copy": lambda: ops.copy(r0, r), "tri": run_tri}
                runs.update({"band%d" % p: run_band(p) for p in ops.LINE_SOLVE_BANDS})
                res = interleaved(runs, lambda run: timed(run, a.inner))
                x.uniform_()                                        # (keep x bounded over the repetitions)
                elems = n * ((W + step - 1) // step) / W            # elements of the addressed systems
                t_copy = float(np.median(res["copy"]))
                out = {"part": "a", "grid": W, "dir": d, "first": first, "step": step, "copy_ms": round(t_copy, 4)}
                t_tri = float(np.median(res["tri"])) - t_copy
                for name, nbytes in (("tri", 64), ("band2", 80), ("band3", 96)):
                    t = float(np.median(res[name])) - t_copy
                    out[name + "_ms"] = round(t, 4)
                    out[name + "_min_ms"] = round(float(res[name].min()) - t_copy, 4)
                    out[name + "_GBps"] = round(nbytes * elems / t / 1e6, 1)
                    out[name + "_vs_tri"] = round(t / t_tri, 3)
                out["byte_model_vs_tri"] = {"band2": 80 / 64, "band3": 96 / 64}
                print(json.dumps(out), flush=True)
        del x, r0, r, tri, facs
        torch.cuda.empty_cache()

if "b" in a.part or "c" in a.part:
    m = a.size
    A, _ = P.anisotropic_poisson_2d_structured(m, 1e-3, 1.0)
    hier = []
    for l, s in enumerate(P.level_sizes(m + 1, a.levels)[:-1]):
        q = P.pseudo_l2_interpolator_1d(s)
        hier.append(P.learned_like(sp.kron(q, q, format="csr"), 43 + l))
    H = Hierarchy(A, hier, dev)
    b = np.random.default_rng(11).standard_normal(A.shape[0])
    b /= np.linalg.norm(b)
    fine = H.levels[0]
    configs = {"line_y": ("Line", 1.0, dict(line_dir="y", line_order="zebra", line_band=3)),
               "line_xy": ("Line", 1.0, dict(line_dir="xy", line_order="zebra", line_band=3)),
               "jacobi": ("Jacobi", 0.8, {})}
    with torch.cuda.stream(H.stream):
        fine.b.copy_(torch.from_numpy(b).to(dev))
        if "b" in a.part:
            runs = {}
            for name, (sm, om, kw) in configs.items():
                H.prepare_smoother(sm, **kw)
                g = H.captured_cycle(sm, 1, om, "lexicographic", **kw)
                runs[name + "_graph"] = g.launch
                runs[name + "_eager"] = (lambda sm=sm, om=om, kw=kw: H.cycle(sm, 1, om, **kw))

            def one(run):
                ops.zero(fine.x)
                return timed(run, a.inner)
            res = interleaved(runs, one)
            out = {"part": "b", "sizes": H.sizes, "bands": [lev.line_band for lev in H.levels[:-1]]}
            for k, v in res.items():
                out[k + "_ms"] = round(float(np.median(v)), 4)
                out[k + "_min_ms"] = round(float(v.min()), 4)
            print(json.dumps(out), flush=True)
        if "c" in a.part:
            for name, (sm, om, kw) in configs.items():
                H.prepare_smoother(sm, **kw)
                g = H.captured_cycle(sm, 1, om, "lexicographic", **kw)
                times, cycles, last = [], 0, 0.0
                for rep in range(3):
                    ops.zero(fine.x)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    cycles = 0
                    last = H.residual_norm(want_vector=False)
                    while last > 1e-8 and cycles < a.max_cycles:
                        g.launch()
                        cycles += 1
                        last = H.residual_norm(want_vector=False)
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t0) * 1e3)
                print(json.dumps({"part": "c", "sizes": H.sizes, "smoother": name, "cycles": cycles, "final_rel_residual": last,
                                  "reached": bool(last <= 1e-8), "ms_median": round(float(np.median(times)), 3),
                                  "ms_min": round(float(min(times)), 3),
                                  "ms_per_cycle": round(float(np.median(times)) / max(cycles, 1), 4)}), flush=True)
