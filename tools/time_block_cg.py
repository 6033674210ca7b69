#!/usr/bin/env python3
"""Multigrid-preconditioned CG on blocks of right-hand sides (CG.solve_many) against m calls of CG.solve with the same
hierarchy, interleaved in one process.

(a) The three kernels alone at k = 2, 4, 8 on n = (cfg3 + 1)^2 rows: ops.block_dot against k launches of ops.dot,
    ops.block_cg_step against k x (two ops.axpby and one ops.dot), ops.block_cg_direction against k launches of ops.axpby.
    Vectors only, the same bytes on both sides up to the |r|^2 the step folds in: what differs is launches and, for the
    step, one pass over r.
(b) Whole solves to 1e-8 |b| at m = 4 and 8 on the cfg#3-like operator (--cfg3: 1441^2 jittered, Dirichlet couplings
    eliminated so that A = A^T, 5 levels, learned-like Q) and on the --size grid (1025^2), V(2,2) at omega = 0.8:
    solve_many against m x CG.solve on one CG object (matrix and hierarchy stay on the device for both).  Columns are
    scaled to |b| = 1.  Wall-clock between synchronisations, host work included -- uploads, the reads per iteration --,
    since that is what a caller waits for.  Per measurement: median and minimum, the iterations, the time per iteration
    (block: per block iteration; singles: per single-column iteration), and the ratio per column.
The baseline is always the single-vector path; block is never compared against block.  One JSON line per measurement; the
byte model of the Krylov side is printed beside the kernel figures (8 B per element read or written).
    python tools/time_block_cg.py --part ab --cfg3 1440 --size 1024"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, scipy.sparse as sp
from learnmultigrid_amd import ops, problems as P
from learnmultigrid_amd.hierarchy import Hierarchy
from learnmultigrid_amd.solvers import CG

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="ab")
ap.add_argument("--cfg3", type=int, default=1440)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--levels", type=int, default=5)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--columns", type=int, nargs="+", default=[4, 8])
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


def wall(run):
    """Milliseconds of one call of run() between two synchronisations."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def interleaved(runs, one):
    """{name: times} over a.reps repetitions (one more is dropped), every candidate once per repetition."""
    res = {k: [] for k in runs}
    for rep in range(a.reps + 1):
        for k, run in runs.items():
            t = one(run)
            if rep: res[k].append(t)
    return {k: np.array(v) for k, v in res.items()}


def symmetric_jittered(m):
    """jittered_poisson_2d(m) with the Dirichlet couplings eliminated: identity rows on the boundary, A = A^T."""
    A, rhs = P.jittered_poisson_2d(m, seed=42)
    A = sp.csr_matrix(A)
    s = m + 1
    idx = np.arange(s * s)
    inter = ((idx % s) > 0) & ((idx % s) < m) & ((idx // s) > 0) & ((idx // s) < m)
    keep = sp.diags(inter.astype(float))
    A = sp.csr_matrix(keep @ A @ keep + sp.diags((~inter).astype(float)))
    A.sort_indices()
    return A, rhs.ravel()


if "a" in a.part:
    n = (a.cfg3 + 1) ** 2
    # bytes per row and column of the Krylov side of one iteration: dot(p, Ap) 16, x and r updates 2 x 24, |r|^2 16 (block:
    # folded into the step), dot(r, z) 16, p update 24
    print("byte model, Krylov side per row and column: singles %d B, block %d B" % (16 + 48 + 16 + 16 + 24, 16 + 48 + 16 + 24))
    x, y, z = (torch.rand(n, dtype=F64, device=dev) for _ in range(3))
    part1 = torch.empty(ops.partials_count(n), dtype=F64, device=dev)
    s1 = torch.zeros(1, dtype=F64, device=dev)
    for k in ops.BLOCK_WIDTHS:
        Pb, AP, X, R, Z = (torch.rand((n, k), dtype=F64, device=dev) for _ in range(5))
        part = torch.empty(ops.block_dot_partials_count(n, k), dtype=F64, device=dev)
        sc = torch.zeros(6 * k, dtype=F64, device=dev)
        rr, mask, tol2, pAp, rz, rz2 = (sc[i * k:(i + 1) * k] for i in range(6))
        mask.fill_(1.0); pAp.fill_(1.0e6); rz.fill_(1.0); rz2.fill_(1.0)     # alpha = 1e-6, beta = 1: nothing grows

        def k_dots():
            for _ in range(k): ops.dot(x, y, part1, s1)

        def k_steps():
            for _ in range(k):
                ops.axpby(1e-6, x, 1.0, y); ops.axpby(-1e-6, x, 1.0, z); ops.dot(z, z, part1, s1)

        def k_dirs():
            for _ in range(k): ops.axpby(1.0, x, 0.5, y)

        runs = {"k_dot": k_dots, "block_dot": lambda: ops.block_dot(Pb, AP, part, pAp),
                "k_step": k_steps, "block_step": lambda: ops.block_cg_step(rz, pAp, tol2, mask, Pb, AP, X, R, part, rr),
                "k_dir": k_dirs, "block_dir": lambda: ops.block_cg_direction(rz, rz2, mask, Z, Pb)}
        res = interleaved(runs, lambda run: timed(run, a.inner))
        for name, bytes_row in (("dot", 16), ("step", 48 + 16), ("dir", 24)):
            ts, tb = float(np.median(res["k_" + name])), float(np.median(res["block_" + name]))
            print(json.dumps({"part": "a", "kernel": name, "n": n, "k": k, "k_singles_ms": round(ts, 4), "block_ms": round(tb, 4),
                              "block_min_ms": round(float(res["block_" + name].min()), 4), "ratio_per_column": round(ts / tb, 3),
                              "block_GBps": round((bytes_row - (16 if name == "step" else 0)) * n * k / tb / 1e6, 1),
                              "singles_GBps": round(bytes_row * n * k / ts / 1e6, 1)}))
        del Pb, AP, X, R, Z
    torch.cuda.empty_cache()

if "b" in a.part:
    for m_grid in (a.cfg3, a.size):
        A, rhs = symmetric_jittered(m_grid)
        hier = []
        for l, s in enumerate(P.level_sizes(m_grid + 1, a.levels)[:-1]):
            base = sp.kron(P.pseudo_l2_interpolator_1d(s), P.pseudo_l2_interpolator_1d(s)).tocsr()
            hier.append(P.learned_like(base, 43 + l))
        H = Hierarchy(A, hier, dev)
        rng = np.random.default_rng(5)
        Ball = np.column_stack([rhs, rng.standard_normal((A.shape[0], max(a.columns) - 1))])
        Ball /= np.linalg.norm(Ball, axis=0)
        cg = CG(A, Ball[:, :1].copy())
        kw = dict(error=1e-8, max_iterations=100, preconditioner=H, precond_steps=2, precond_omega=0.8)
        fine = [t for t in ("stencil", "patterns", "sell", "packed", "dia") if getattr(H.levels[0].A, t, None) is not None]
        for m in a.columns:
            B = np.ascontiguousarray(Ball[:, :m])

            def singles():
                its, X = 0, np.empty_like(B)
                for j in range(m):
                    cg.rhs = B[:, j:j + 1]
                    cg.iterations = 0
                    cg.solve(**kw)
                    its += cg.get_iterations()
                    X[:, j] = cg.get_solution()[:, 0]
                return its, X

            def block():
                X, track = cg.solve_many(B, **kw)
                return int(cg.iterations_many.max()), X

            def block_graph():
                X, track = cg.solve_many(B, use_graph=True, **kw)
                return int(cg.iterations_many.max()), X

            outs = {}

            def one(run):
                t, outs[run.__name__] = wall(run)
                return t
            res = interleaved({"singles": singles, "block": block, "block_graph": block_graph}, one)
            (its_s, Xs), (its_b, Xb) = outs["singles"], outs["block"]
            ts, tb, tg = (float(np.median(res[k])) for k in ("singles", "block", "block_graph"))
            print(json.dumps({"part": "b", "sizes": H.sizes, "m": m, "fine_twins": fine,
                              "singles_ms": round(ts, 3), "singles_min_ms": round(float(res["singles"].min()), 3),
                              "singles_iterations_total": its_s, "singles_ms_per_iteration": round(ts / its_s, 4),
                              "block_ms": round(tb, 3), "block_min_ms": round(float(res["block"].min()), 3),
                              "block_iterations": its_b, "block_ms_per_iteration": round(tb / its_b, 4),
                              "block_graph_ms": round(tg, 3), "ratio_to_tolerance": round(ts / tb, 3),
                              "ratio_to_tolerance_graph": round(ts / tg, 3),
                              "ratio_per_column_iteration": round((ts / its_s) / (tb / its_b / m), 3),
                              "max_rel_diff_of_solutions": float(np.abs(Xs - Xb).max() / np.abs(Xs).max())}))
        del H, cg
        torch.cuda.empty_cache()
