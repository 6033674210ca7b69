#!/usr/bin/env python3
"""The multi-right-hand-side path against the single-vector path it amortises, interleaved in one process.

(a) Jacobi sweep: ops.block_jacobi at k = 2, 4, 8 against k launches of ops.csr_jacobi on the same sliced-ELL twin, on
    the Galerkin operators of the cfg#5-style hierarchy tools/time_sell.py builds (--size 4096: 2049^2 x 25 entries and
    1025^2 x 49 entries).
(b) One cycle: a BlockCycle V(2,2) cycle at k = 4 against 4 x H.cycle("Jacobi", 2, 0.8) on cfg#3 (1441^2 jittered, 5 levels,
    learned-like Q).
The baseline is always the single-vector path; block is never compared against block.  Prints one line per measurement:
median and minimum time, the ratio per column, and the ratio of the byte model (10 B per entry + 4 B per row of matrix,
24 B per row and column of vectors).
    python tools/time_block.py --part ab --size 4096 --cfg3 1440"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, scipy.sparse as sp
from learnmultigrid_amd import ops, problems as P
from learnmultigrid_amd.block import BlockCycle
from learnmultigrid_amd.hierarchy import Hierarchy

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="ab")
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--cfg3", type=int, default=1440)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=10)
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


def interleaved(runs, inner):
    """{name: times} over a.reps repetitions (one more is dropped), every candidate once per repetition."""
    res = {k: [] for k in runs}
    for rep in range(a.reps + 1):
        for k, run in runs.items():
            t = timed(run, inner)
            if rep: res[k].append(t)
    return {k: np.array(v) for k, v in res.items()}


def galerkin_operators(m):
    """The level-1 and level-2 Galerkin operators of time_sell.py's hierarchy, by the device SpGEMM."""
    M = ops.DeviceCSR.from_scipy(P.variable_coeff_poisson_2d_structured(m, seed=44)[0], dev)
    out = []
    for li, sz in enumerate(P.level_sizes(m + 1, 3)[:2]):
        l2 = P.pseudo_l2_interpolator_1d(sz)
        Q = ops.DeviceCSR.from_scipy(P.learned_like(sp.kron(l2, l2).tocsr(), 43 + li), dev)
        M = ops.spgemm(ops.spgemm(Q.transpose(), M), Q)
        out.append(M)
    return out


def model_ratio(entries, k):
    """Bytes per column of k single sweeps over bytes per column of one block sweep, per row."""
    return (10 * entries + 4 + 24) / ((10 * entries + 4 + 24 * k) / k)


if "a" in a.part:
    for dM in galerkin_operators(a.size):
        n = dM.shape[0]
        dM.sell = ops.SellCSR.from_csr(dM, max_padding=float("inf"))
        S = ops.block_twin(dM)
        assert S is dM.sell
        L = dM.nnz / n
        x, b = torch.rand(n, dtype=F64, device=dev), torch.rand(n, dtype=F64, device=dev)
        y = torch.zeros_like(x)
        runs = {"single": lambda: ops.csr_jacobi(dM, x, b, 0.8, y)}
        blocks = {}
        for k in ops.BLOCK_WIDTHS:
            blocks[k] = (torch.rand((n, k), dtype=F64, device=dev), torch.rand((n, k), dtype=F64, device=dev),
                         torch.zeros((n, k), dtype=F64, device=dev))
            runs["block%d" % k] = (lambda X, B, Y: (lambda: ops.block_jacobi(S, X, B, 0.8, Y)))(*blocks[k])
        res = interleaved(runs, a.inner)
        t1 = float(np.median(res["single"]))
        print("sweep n %d (%d^2) entries/row %.1f max_len %d colmode %d: single median %.4f ms min %.4f" %
              (n, int(round(n ** 0.5)), L, S.max_len, S.colmode, t1, res["single"].min()))
        for k in ops.BLOCK_WIDTHS:
            tk = float(np.median(res["block%d" % k]))
            print(json.dumps({"part": "a", "n": n, "entries_per_row": round(L, 2), "k": k, "single_ms": round(t1, 4),
                              "k_singles_ms": round(k * t1, 4), "block_ms": round(tk, 4), "block_min_ms": round(float(res["block%d" % k].min()), 4),
                              "ratio_per_column": round(k * t1 / tk, 3), "byte_model_ratio": round(model_ratio(S.max_len, k), 3)}))
        del blocks, runs, dM, S
        torch.cuda.empty_cache()

if "b" in a.part:
    m, levels, k = a.cfg3, 5, 4
    A, rhs = P.jittered_poisson_2d(m, seed=42)
    hier = []
    for l, s in enumerate(P.level_sizes(m + 1, levels)[:-1]):
        base = sp.kron(P.pseudo_l2_interpolator_1d(s), P.pseudo_l2_interpolator_1d(s)).tocsr()
        hier.append(P.learned_like(base, 43 + l))
    H = Hierarchy(A, hier, dev)
    rng = np.random.default_rng(5)
    B = np.column_stack([rhs.ravel(), rng.standard_normal((A.shape[0], k - 1))])
    with torch.cuda.stream(H.stream):
        bc = BlockCycle(H, k)
        bc.levels[0].b.copy_(torch.from_numpy(B).to(dev))
        H.levels[0].b.copy_(torch.from_numpy(np.ascontiguousarray(B[:, 0])).to(dev))
        # what is timed computes the same thing: column 0 of the block cycle against the single-vector cycle (the fine
        # level runs other kernels there: agreement to rounding, not to the bit)
        bc.cycle(2, 0.8); H.cycle("Jacobi", 2, 0.8)
        x0, x1 = bc.levels[0].x[:, 0].cpu().numpy(), H.levels[0].x.cpu().numpy()
        print("cycle check: max |block column 0 - single| / max |single| = %.2e" % (np.abs(x0 - x1).max() / np.abs(x1).max()))

        def singles():
            for _ in range(k): H.cycle("Jacobi", 2, 0.8)
        res = interleaved({"single_x%d" % k: singles, "block%d" % k: lambda: bc.cycle(2, 0.8)}, max(a.inner // 2, 1))
    ts, tb = float(np.median(res["single_x%d" % k])), float(np.median(res["block%d" % k]))
    print(json.dumps({"part": "b", "sizes": H.sizes, "k": k, "k_single_cycles_ms": round(ts, 4), "k_single_min_ms": round(float(res["single_x%d" % k].min()), 4),
                      "block_cycle_ms": round(tb, 4), "block_min_ms": round(float(res["block%d" % k].min()), 4), "ratio_per_column": round(ts / tb, 3),
                      "fine_twins": [t for t in ("stencil", "patterns", "sell", "packed", "dia") if getattr(H.levels[0].A, t, None) is not None]}))
