"""TEST-ONLY plain-Python restatement of the rules of smoothed aggregation for systems ("Smoothed
aggregation for systems"): the condensation of node blocks, the tentative prolongator of k candidates by two rounds of
Cholesky-QR per aggregate, and the level loop that carries (candidate, block size) from level to level.  Written from the
rules, entry by entry, with no care for speed: what learnmultigrid_amd/aggregation.py and csrc/nsp.hip are compared with,
integer for integer and bit for bit (every product and every sum rounds on its own, every sum starts from 0.0 and runs in
the order stated).  Strength, graph, MIS-2 roots, aggregates, the Jacobi step and the Galerkin product are those of
tests/sa_ref.py.  Nothing in learnmultigrid_amd imports this file.

Matrices are SciPy CSR with sorted, duplicate-free rows; explicit zeros stay where they are."""
import numpy as np
import scipy.sparse as sp

import sa_ref as S
from amg_ref import Refused, canonical, galerkin, row_of

K_MAX = 6
F = np.float64


def condense(A, bs):
    """C (N x N, N = n / bs): an entry (I, J) iff some stored a_ij lies in that block (explicit zeros count), columns
    ascending, c_IJ = sqrt(sum a_ij a_ij) over the rows of the block ascending and in storage order within a row."""
    A = canonical(A)
    n = A.shape[0]
    if bs < 1 or n % bs:
        raise ValueError("block_size")
    if bs == 1:
        return A
    N = n // bs
    indptr, indices, data = [0], [], []
    for I in range(N):
        rows = [row_of(A, bs * I + r) for r in range(bs)]
        for J in sorted({j // bs for cols, _ in rows for j in cols}):
            s = F(0.0)
            for cols, vals in rows:
                for j, v in zip(cols, vals):
                    if j // bs == J:
                        s = s + F(v) * F(v)
            indices.append(J)
            data.append(float(np.sqrt(s)))
        indptr.append(len(indices))
    return sp.csr_matrix((np.array(data, dtype=F), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)),
                         shape=(N, N))


def candidates(B, n, bs):
    """The candidates as an (n, k) array; None: ones for bs = 1, else the bs unit translations."""
    if B is None:
        if bs == 1:
            return np.ones((n, 1))
        X = np.zeros((n, bs))
        X[np.arange(n), np.arange(n) % bs] = 1.0
        return X
    X = np.asarray(B, dtype=F)
    X = X.reshape(-1, 1) if X.ndim == 1 else X
    if X.shape[0] != n or not 1 <= X.shape[1] <= K_MAX:
        raise ValueError("candidates")
    return np.ascontiguousarray(X)


def members(agg, n_agg, bs):
    """Per aggregate the member rows: those of its nodes ascending, the unknowns within a node ascending."""
    out = [[] for _ in range(n_agg)]
    for I, a in enumerate(agg):
        if a >= 0:
            out[a].extend(range(bs * I, bs * I + bs))
    return out


def gram_chol(X, rows, rank_tol):
    """(R or None, pivot ratios): the upper Cholesky factor (k x k, zeros below) of the Gram matrix of the rows `rows` of X;
    None where a pivot s is not finite or not above rank_tol g_cc."""
    k = X.shape[1]
    g = [[F(0.0)] * k for _ in range(k)]
    for i in rows:
        for p in range(k):
            for q in range(p, k):
                g[p][q] = g[p][q] + X[i, p] * X[i, q]
    R = [[F(0.0)] * k for _ in range(k)]
    ratios = []
    for c in range(k):
        for r in range(c + 1):
            s = g[r][c]
            for q in range(r):
                s = s - R[q][r] * R[q][c]
            if r < c:
                R[r][c] = s / R[r][r]
            else:
                if not (np.isfinite(s) and s > F(rank_tol) * g[c][c]):
                    return None, ratios
                ratios.append(float(s / g[c][c]))
                R[c][c] = np.sqrt(s)
    return np.array(R, dtype=F), ratios


def apply_row(x, R):
    """y = x R^-1 by forward substitution: y_c = (x_c - y_0 R_0c - ... - y_(c-1) R_(c-1)c) / R_cc."""
    k = len(x)
    y = [F(0.0)] * k
    for c in range(k):
        t = F(x[c])
        for q in range(c):
            t = t - y[q] * R[q, c]
        y[c] = t / R[c, c]
    return y


def tri_product(R2, R1):
    k = R1.shape[0]
    out = np.zeros((k, k))
    for r in range(k):
        for c in range(r, k):
            s = F(0.0)
            for q in range(r, c + 1):
                s = s + R2[r, q] * R1[q, c]
            out[r, c] = s
    return out


def _round(X, mem, bs, rank_tol, agg_nodes, ratios):
    """One round of Cholesky-QR on every aggregate: (Y, [R_j]); refuses with the smallest row of a refused aggregate."""
    Rs, bad = [], []
    for j, rows in enumerate(mem):
        R, rat = gram_chol(X, rows, rank_tol)
        ratios.extend(rat)
        Rs.append(R)
        if R is None:
            bad.append(rows[0] if rows else 0)
    if bad:
        raise Refused("candidate", min(bad))
    Y = np.zeros_like(X)
    for j, rows in enumerate(mem):
        for i in rows:
            Y[i] = apply_row(X[i], Rs[j])
    return Y, Rs


def tentative(agg, n_agg, bs, X, rank_tol=1e-12, ratios=None):
    """(T, Bc): T (n x k n_agg), every aggregated row with k entries at columns k agg + c, c ascending, the row of Q;
    Bc (k n_agg x k) the blocks R' R, upper triangular.  agg: per NODE."""
    X = np.asarray(X, dtype=F)
    n, k = X.shape
    ratios = [] if ratios is None else ratios
    mem = members(agg, n_agg, bs)
    with np.errstate(all="ignore"):
        Y, R1 = _round(X, mem, bs, rank_tol, agg, ratios)
        Q, R2 = _round(Y, mem, bs, rank_tol, agg, ratios)
        Bc = np.zeros((k * n_agg, k))
        for j in range(n_agg):
            Bc[k * j:k * j + k] = tri_product(R2[j], R1[j])
    indptr, indices, data = [0], [], []
    for i in range(n):
        a = agg[i // bs]
        if a >= 0:
            indices.extend(k * int(a) + c for c in range(k))
            data.extend(float(v) for v in Q[i])
        indptr.append(len(indices))
    T = sp.csr_matrix((np.array(data, dtype=F), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)),
                      shape=(n, k * n_agg))
    return T, Bc


def transfer(A, X, theta=0.0, omega=4.0 / 3.0, bs=1, rank_tol=1e-12):
    """(P or None, Bc or None, info, parts) of one level on the new path; None where the aggregation gives no coarse level
    (n_agg = 0 or n_agg = N, the number of nodes).  parts: C, S, G, state, agg (per node), rows (agg per unknown), T."""
    A = canonical(A)
    n = A.shape[0]
    C = condense(A, bs)
    St = S.symmetric_strength(C, theta)
    agg, n_agg, rounds, state, G = S.aggregate(St)
    info = {"n": n, "nnz": A.nnz, "n_agg": n_agg, "rounds": rounds}
    rows = np.repeat(agg, bs)
    parts = {"C": C, "S": St, "G": G, "state": state, "agg": agg, "rows": rows, "ratios": []}
    if n_agg == 0 or n_agg == C.shape[0]:
        return None, None, info, parts
    T, Bc = tentative(agg, n_agg, bs, X, rank_tol, parts["ratios"])
    parts["T"] = T
    return S.smooth_prolongator(A, T, rows, omega), Bc, info, parts


def sa_transfers(A, theta=0.0, B=None, omega=4.0 / 3.0, block_size=1, rank_tol=1e-12, max_levels=10, max_coarse=500):
    """([P_0, ...], [A_0, ...], info) as sa_ref.sa_transfers, for k candidates on node blocks: the level loop carries
    (candidate, block size) -- block_size on the fine level, k below it.  k = 1 with block size 1 is sa_ref's own path.
    info gains block_size and candidates per aggregated level."""
    A = canonical(A)
    X, bs = candidates(B, A.shape[0], block_size), int(block_size)
    Ps, As, infos = [], [A], []
    while len(As) < max_levels and As[-1].shape[0] > max_coarse:
        k = X.shape[1]
        if k == 1 and bs == 1:
            P, Bc, info, _ = S.transfer(As[-1], X.ravel(), theta, omega)
            Bc = None if Bc is None else Bc.reshape(-1, 1)
        else:
            P, Bc, info, _ = transfer(As[-1], X, theta, omega, bs, rank_tol)
        infos.append(dict(info, block_size=bs, candidates=k))
        if P is None:
            break
        Ps.append(P)
        As.append(galerkin(As[-1], P))
        X, bs = Bc, k
    return Ps, As, infos
