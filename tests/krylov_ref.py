"""TEST-ONLY CPU twin of learnmultigrid_amd/krylov.py in NumPy: right-preconditioned flexible GMRES(m) with classical
Gram-Schmidt applied twice, Givens rotations, and the same `track` contract -- entry 0 the true initial residual norm, one
Arnoldi estimate per inner iteration, the last one of every cycle replaced by the recomputed true norm."""
import math

import numpy as np


def fgmres_ref(A, b, M=None, restart=30, max_iterations=1000, error=1e-8, x0=None):
    """A: scipy sparse or dense matrix; M(v) -> z, a callable that may change from call to call, or None.
    Returns (x, track, iterations)."""
    b = np.asarray(b, dtype=float).reshape(-1)
    n = b.size
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=float).reshape(-1)
    m = int(restart)
    r = b - A @ x
    beta = math.sqrt(float(r @ r))
    track = [beta]
    its = 0
    while beta > error and beta > 0.0 and its < max_iterations:
        V = np.zeros((m + 1, n))
        Z = np.zeros((m, n))
        V[0] = (1.0 / beta) * r
        Hm = np.zeros((m + 1, m))              # the Hessenberg matrix, rotated into a triangle column by column
        g = np.zeros(m + 1)
        g[0] = beta
        cs, sn = np.zeros(m), np.zeros(m)
        k = 0
        for j in range(m):
            if its == max_iterations:
                break
            Z[j] = V[j] if M is None else M(V[j])
            w = A @ Z[j]
            h1 = V[:j + 1] @ w
            for i in range(j + 1):
                w = w - h1[i] * V[i]
            h2 = V[:j + 1] @ w
            for i in range(j + 1):
                w = w - h2[i] * V[i]
            hn = math.sqrt(float(w @ w))
            Hm[:j + 1, j] = h1 + h2
            its += 1
            k = j + 1
            for i in range(j):
                t = cs[i] * Hm[i, j] + sn[i] * Hm[i + 1, j]
                Hm[i + 1, j] = -sn[i] * Hm[i, j] + cs[i] * Hm[i + 1, j]
                Hm[i, j] = t
            d = math.hypot(Hm[j, j], hn)
            cs[j], sn[j] = (1.0, 0.0) if d == 0.0 else (Hm[j, j] / d, hn / d)
            Hm[j, j] = cs[j] * Hm[j, j] + sn[j] * hn
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            track.append(abs(g[j + 1]))
            if track[-1] <= error or hn == 0.0:
                break
            V[j + 1] = (1.0 / hn) * w
        y = np.zeros(k)
        for i in range(k - 1, -1, -1):
            t = g[i] - Hm[i, i + 1:k] @ y[i + 1:]
            y[i] = t / Hm[i, i] if Hm[i, i] != 0.0 else 0.0
        for i in range(k):
            x = x + y[i] * Z[i]
        r = b - A @ x
        beta = math.sqrt(float(r @ r))
        track[-1] = beta
    return x, track, its
