#!/usr/bin/env python3
"""Generate tests/golden/g8_nmg2d_<case>.npz by RUNNING the reference's NeuralMG_2D stage by stage
(learn_multigrid/solvers/Multigrid.py:373-765) in the build container, like tools/make_golden.py does for the other
fixtures (its stand-in modules are reused).  The files hold data only, per level l:
    CC, patches, fill_idxs, res (the stored predictions, float32 values), B (COO) and Q's values on B's pattern,
    d_neighs (n_c x 6, padded with -1), Mc = (Q^T M) Q (COO) and the mask of its entries that pre_process(Mc, d_neighs) keeps
plus M of level 0 (COO; the M of a later level is the kept part of the Mc before it), mean, std, levels and, for the
solve case k16, A and rhs.

The "model" of every case is a table: res = 0.2 + 0.1 u (seeded, rounded to float32), so positive, and no BLAS or
tanh is evaluated on two machines; what it is shown is (patches - mean) / std, which a test recomputes from the stored
patches (element-wise IEEE operations).

Usage:  python tools/make_golden_nmg2d.py"""
import os
import sys

import numpy as np
import scipy.sparse as sp
from scipy.sparse import lil_matrix

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (installs the stand-ins, then imports the reference)

with G.contextlib.redirect_stdout(G.io.StringIO()):
    from learn_multigrid.solvers.Multigrid import NeuralMG_2D  # noqa: E402

# three extra symmetric edges across cell diagonals of the 17 x 17 mesh: six nodes of valence 7, two of them coarse
VALENCE7_EDGES = ((57, 73), (218, 234), (38, 54))


def load_mass(k):
    g = np.load(os.path.join(G.OUT, "g4_structured2d_k%d.npz" % k))
    shape = tuple(int(s) for s in g["M_shape"])
    M = sp.coo_matrix((g["M_data"], (g["M_row"], g["M_col"])), shape=shape).tocsr()
    A = sp.coo_matrix((g["A_data"], (g["A_row"], g["A_col"])), shape=shape).tocsr()
    return M, A, g["rhs"]


def jitter(M, seed):
    """Every entry scaled by 0.7 + 0.6 u, the same factor for (i, j) and (j, i): distinct values, same pattern."""
    C = sp.coo_matrix(M)
    n = M.shape[0]
    rng = np.random.RandomState(seed)
    lo, hi = np.minimum(C.row, C.col).astype(np.int64), np.maximum(C.row, C.col).astype(np.int64)
    pair, inv = np.unique(lo * n + hi, return_inverse=True)
    f = 0.7 + 0.6 * rng.random_sample(pair.size)
    return sp.csr_matrix((C.data * f[inv], (C.row, C.col)), shape=M.shape)


def valence7(M):
    L = M.tolil()
    for e, (a, b) in enumerate(VALENCE7_EDGES):
        assert L[a, b] == 0 and L[b, a] == 0
        L[a, b] = L[b, a] = 0.4 * M[a, a] * (1 + 0.1 * e) / 6
    return L.tocsr()


def renumber(M, seed):
    perm = np.random.RandomState(seed).permutation(M.shape[0])
    return sp.csr_matrix(M[perm][:, perm])


def run_case(name, M, levels, seed, mean, std, expect, A=None, rhs=None):
    n = M.shape[0]
    nmg = G.quiet(NeuralMG_2D, sp.identity(n, format="csc"), np.zeros((n, 1)), None, None, std, mean)
    rng = np.random.RandomState(seed)
    arrs = dict(levels=levels, mean=mean, std=std)
    if A is not None:
        arrs.update(G.coo(A, "A"), rhs=rhs)
    mass = lil_matrix(M)
    d_neighs, counts = {}, []
    for lev in range(levels - 1):
        if d_neighs:
            mass = nmg.pre_process(mass, d_neighs)
        before = mass.copy()
        C, _F, _Cn, _Fn = G.quiet(nmg.coarsening, mass)
        assert (before != mass).nnz == 0                    # coarsening works on a copy
        mapp = nmg.map_coarse(C)
        patches, idx = G.quiet(nmg.extract_patches, C, mass)
        res = (0.2 + 0.1 * rng.random_sample((patches.shape[0], 31))).astype(np.float32).astype(np.float64)
        B, d_neighs = G.quiet(nmg.fill_B, res, idx, mass.shape[0], mapp, C)
        row_sums = B.sum(axis=1)
        Q = lil_matrix(B / row_sums[:, np.newaxis])
        Mc = lil_matrix(Q.T @ mass @ Q)
        dn = -np.ones((len(C), 6), dtype=np.int64)
        for r in range(len(C)):
            dn[r, :len(d_neighs[r])] = d_neighs[r]
        pre = "l%d_" % lev
        # B and Q share a pattern, the cut keeps a subset of Mc's entries, and the next level's M is that subset: stored once
        Bs, Qs, Mcs = sp.csr_matrix(B), sp.csr_matrix(Q), sp.coo_matrix(sp.csr_matrix(Mc))
        assert np.array_equal(Bs.indptr, Qs.indptr) and np.array_equal(Bs.indices, Qs.indices)
        cut = sp.csr_matrix(nmg.pre_process(Mc, d_neighs))
        keep = np.asarray(cut[Mcs.row, Mcs.col]).ravel() != 0
        assert keep.sum() == cut.nnz and np.array_equal(np.asarray(cut[Mcs.row, Mcs.col]).ravel()[keep], Mcs.data[keep])
        if lev == 0:
            arrs.update(G.coo(mass, pre + "M"))
        arrs.update(G.coo(Bs, pre + "B"), **{pre + "Q_data": Qs.data, pre + "Mcut_keep": keep})
        arrs.update(G.coo(Mcs, pre + "Mc"))
        assert np.array_equal(res, res.astype(np.float32).astype(np.float64))
        arrs.update({pre + "CC": np.asarray(C, dtype=np.int32), pre + "patches": patches, pre + "fill_idxs": idx.astype(np.int32),
                     pre + "res": res.astype(np.float32), pre + "d_neighs": dn.astype(np.int32)})
        counts.append((len(C), patches.shape[0]))
        mass = Mc
    assert counts[0][0] in expect[0] and counts[0][1] in expect[1], counts
    G.save("g8_nmg2d_" + name, **arrs)
    print("   coarse nodes / patches per level:", counts)
    assert os.path.getsize(os.path.join(G.OUT, "g8_nmg2d_%s.npz" % name)) < 100 * 1024


if __name__ == "__main__":
    ones, zeros = np.ones(43), np.zeros(43)
    M4, _A4, _r4 = load_mass(4)
    M16, A16, rhs16 = load_mass(16)
    run_case("k4", M4, 2, 801, zeros, ones, ((9,), (9,)))
    run_case("k16", M16, 3, 802, zeros, ones, ((81,), (81,)), A=A16, rhs=rhs16)
    Mj = jitter(M16, 803)
    run_case("k16_jitter", Mj, 3, 804, 1e-4 * (1.0 + 0.1 * np.arange(43)), 1e-3 * (1.0 + 0.05 * np.arange(43)),
             ((81,), (81,)))
    run_case("k16_valence7", valence7(Mj), 3, 805, zeros, ones, ((81,), (83,)))
    # (two levels: the greedy split of a randomly numbered mesh leaves coarse graphs the patch rules refuse)
    run_case("k16_random", renumber(M16, 809), 2, 807, zeros, ones, ((71, 72), (71, 72)))
