#!/usr/bin/env python3
"""fp32 against fp64 value streams of the same matrix, interleaved in one process, with a second fp64 twin of that matrix in
the same run to show the spread (A/A).  Kernels:
    python tools/time_f32_values.py sell --size 4096 --matrix L1      Jacobi sweep and residual, 25-entry Galerkin level
    python tools/time_f32_values.py sell --size 4096 --matrix L2      the same on the ~48-entry level
    python tools/time_f32_values.py dia --size 4096                   3 sweeps + residual in one pass, 4097^2
    python tools/time_f32_values.py dia --size 1024
whole solves on the cfg#5-style hierarchy (variable coefficients, learned-like L2-type transfers):
    python tools/time_f32_values.py cycle --size 4096 --levels 5      one V(2,2) Jacobi cycle, replayed from a hipGraph
    python tools/time_f32_values.py gmres --size 4096 --levels 5      GMRES(30) to --rtol (1e-10) relative: time and iterations"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, scipy.sparse as sp
from learnmultigrid_amd import ops, problems as P
from learnmultigrid_amd.hierarchy import Hierarchy

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=("sell", "dia", "cycle", "gmres"))
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--matrix", default="L1")
ap.add_argument("--levels", type=int, default=5)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--rtol", type=float, default=1e-10, help="gmres: relative residual to reach")
a = ap.parse_args()
m, dev = a.size, "cuda:0"
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def transfers(levels):
    out = []
    for li, sz in enumerate(P.level_sizes(m + 1, levels)[:-1]):
        l2 = P.pseudo_l2_interpolator_1d(sz)
        out.append(P.learned_like(sp.kron(l2, l2).tocsr(), 43 + li))
    return out


def interleaved(runs, inner=10, streams=None):
    """runs: {label: callable}; median / min ms per call over a.reps rounds, the labels taking turns inside a round.
    streams: {label: the stream its launches go to} (the events are recorded there), None = the current stream."""
    res = {k: [] for k in runs}
    for rep in range(a.reps + 1):
        for k, fn in runs.items():
            st = torch.cuda.current_stream() if streams is None else streams[k]
            fn(); torch.cuda.synchronize()
            ev0.record(st)
            for _ in range(inner): fn()
            ev1.record(st); torch.cuda.synchronize()
            if rep: res[k].append(ev0.elapsed_time(ev1) / inner)
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in res.items()}


def report(title, t, model=None):
    base = t["f64"][0]
    for k, (med, mn) in t.items():
        bw = "" if model is None else "  %.0f GB/s on the byte model" % (model[k] / med / 1e6)
        print("%-22s %-6s median %.4f ms  min %.4f  f64/this %.3f%s" % (title, k, med, mn, base / med, bw))


M, rhs = P.variable_coeff_poisson_2d_structured(m, seed=44)
if a.what == "sell":
    for Q in transfers(3)[:2 if a.matrix == "L2" else 1]:
        M = sp.csr_matrix(Q.T @ M @ Q)
    M.sort_indices()
    n = M.shape[0]
    tw = {}
    for k, v in (("f64", "f64"), ("f64'", "f64"), ("f32", "f32")):
        d = ops.DeviceCSR.from_scipy(M, dev)
        d.pack(values=v)
        assert d.sell is not None and d.sell.values == v, "pack() chose no sliced-ELL twin of that width"
        tw[k] = d
    S = tw["f32"].sell
    print("matrix %s n %d nnz/row %.1f padded/nnz %.3f colmode %d" % (a.matrix, n, M.nnz / n, S.padded / M.nnz, S.colmode))
    cb = (2, 4)[S.colmode]
    model = {k: ((cb + (4 if k == "f32" else 8)) * M.nnz + 24 * n) for k in tw}
    x = torch.rand(n, dtype=torch.float64, device=dev); b = torch.rand_like(x); y = torch.zeros_like(x)
    report("jacobi", interleaved({k: (lambda d=d: ops.csr_jacobi(d, x, b, 0.8, y)) for k, d in tw.items()}), model)
    report("residual", interleaved({k: (lambda d=d: ops.csr_residual_norm2(d, x, b, y, None, None)) for k, d in tw.items()}), model)
elif a.what == "dia":
    M = sp.csr_matrix(M); M.sort_indices()
    n = M.shape[0]
    tw = {}
    for k, v in (("f64", "f64"), ("f64'", "f64"), ("f32", "f32")):
        d = ops.DeviceCSR.from_scipy(M, dev)
        d.pack(values=v)
        assert d.dia is not None and d.dia.values == v
        tw[k] = d
    ns = tw["f32"].dia.nslots
    print("n %d slots %d" % (n, ns))
    model = {k: ((4 if k == "f32" else 8) * ns * n + 32 * n) for k in tw}       # single pass: slots + x, b in, x, r out
    x = torch.rand(n, dtype=torch.float64, device=dev); b = torch.rand_like(x); y = torch.zeros_like(x); r = torch.zeros_like(x)
    report("3 sweeps + residual", interleaved({k: (lambda d=d: ops.stencil_smooth(d, x, b, 0.8, 3, y, r)) for k, d in tw.items()}), model)
    report("2 sweeps", interleaved({k: (lambda d=d: ops.stencil_smooth(d, x, b, 0.8, 2, y, None)) for k, d in tw.items()}), model)
else:
    hier = transfers(a.levels)
    A = sp.csr_matrix(M)
    Hs = {}
    for k, v in (("f64", "f64"), ("f64'", "f64"), ("f32", "f32")):
        if a.what == "gmres" and k == "f64'":
            continue
        t0 = time.perf_counter()
        Hs[k] = Hierarchy(A, hier, dev, cycle_values=v)
        torch.cuda.synchronize()
        print("%-5s setup %.2f s  twin bytes %.1f MB  cycle bytes V(2,2) %.1f MB" % (
            k, time.perf_counter() - t0, Hs[k].twin_bytes() / 1e6, Hs[k].cycle_bytes(2)[0] / 1e6))
    if a.what == "cycle":
        runs = {}
        for k, H in Hs.items():
            with torch.cuda.stream(H.stream):
                H.levels[0].b.copy_(torch.from_numpy(rhs.ravel().copy()).to(dev))
                g = H.captured_cycle("Jacobi", 2, 0.8, "lexicographic")
            def run(H=H, g=g):
                with torch.cuda.stream(H.stream):
                    g.launch()
            runs[k] = run
        report("V(2,2) cycle", interleaved(runs, inner=5, streams={k: H.stream for k, H in Hs.items()}))
    else:
        from learnmultigrid_amd.solvers import GMRES
        b = rhs.ravel()
        tol = a.rtol * np.linalg.norm(b)
        for rep in range(3):
            for k, H in Hs.items():
                s = GMRES(A, b.copy())
                torch.cuda.synchronize(); t0 = time.perf_counter()
                s.solve(max_iterations=1500, error=tol, restart=30, preconditioner=H, precond_steps=2, precond_omega=0.8)
                torch.cuda.synchronize(); dt = time.perf_counter() - t0
                rel = np.linalg.norm(b - A @ s.get_solution().ravel()) / np.linalg.norm(b)
                print("GMRES(30) %-5s run %d  %.1f ms  %d iterations  true relative residual %.2e" % (k, rep, 1e3 * dt, s.get_iterations(), rel))
