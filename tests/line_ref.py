"""CPU restatement of the line relaxation smoother and of the cycles that use it -- TEST INFRASTRUCTURE ONLY.

Plain NumPy, vectorised across the systems of a direction, written from the definition.  A level has n rows and a line
stride W, n = H W.  Direction "x": one system per storage line y, rows y W .. y W + W - 1, matrix T = the entries of A at
column - row in {-1, 0, +1}; direction "y": one system per grid column k, rows k, k + W, ..., the entries at
column - row in {-W, 0, +W}; a missing entry is 0.  Factorisation along a system j = 0 .. L - 1 (lo, a, up its sub-, main
and super-diagonal), once:
    den_0 = a_0,  den_j = a_j - lo_j cp_(j-1),  minv_j = 1.0 / den_j,  cp_j = up_j minv_j,
solve, per half-sweep, products and sums rounded separately:
    d_0 = r_0 minv_0,  d_j = (r_j - lo_j d_(j-1)) minv_j,  e_(L-1) = d_(L-1),  e_j = d_j - cp_j e_(j+1),  x = x + omega e_j.
One half-sweep is x <- x + omega T^-1 (b - A x) on a set of systems; "zebra" runs the even systems then the odd ones with a
fresh residual in between, "jacobi" all from one residual; "xy" is an x half-step then a y half-step.  The post-smoothing
half of a cycle runs directions and colours in reverse.  The residual is the oracle's (storage-order row sums).
"""
import numpy as np
import scipy.sparse as sp

from oracle import kernels as K

CHILDREN = {"V": ("V",), "W": ("W", "W"), "F": ("F", "V")}
COUPLED, PIVOT = 1, 2


def by_system(v, W, direction):
    """The n-vector v as a [system, element] VIEW."""
    g = v.reshape(-1, W)
    return g if direction == "x" else g.T


def tridiagonals(A, W, direction):
    """(lo, a, up, flags): three n-vectors indexed by row; flags has COUPLED set if, in direction x, a stored non-zero
    entry couples two lines (those entries belong to no system)."""
    A = K.as_csr(A)
    n = A.shape[0]
    assert n % W == 0
    s = 1 if direction == "x" else W
    coo = A.tocoo()
    off = coo.col.astype(np.int64) - coo.row
    out = []
    for k in (-s, 0, s):
        v = np.zeros(n)
        m = off == k
        v[coo.row[m]] = coo.data[m]
        out.append(v)
    lo, a, up = out
    flags = 0
    if direction == "x":
        first, last = np.arange(0, n, W), np.arange(W - 1, n, W)
        if np.any(lo[first] != 0) or np.any(up[last] != 0):
            flags |= COUPLED
        lo[first] = 0.0
        up[last] = 0.0
    return lo, a, up, flags


def factor(A, W, direction):
    """((lo, minv, cp), flags) -- n-vectors indexed by row; PIVOT set if a pivot is zero or not finite."""
    lo, a, up, flags = tridiagonals(A, W, direction)
    minv, cp = np.empty_like(a), np.empty_like(a)
    L, A_, U, M, C = (by_system(v, W, direction) for v in (lo, a, up, minv, cp))
    bad = False
    with np.errstate(all="ignore"):
        for j in range(A_.shape[1]):
            den = A_[:, j] if j == 0 else A_[:, j] - L[:, j] * C[:, j - 1]
            bad |= bool(np.any((den == 0) | ~np.isfinite(den)))
            M[:, j] = 1.0 / den
            C[:, j] = U[:, j] * M[:, j]
    return (lo, minv, cp), flags | (PIVOT if bad else 0)


def solve(fac, W, direction, first, step, r, omega, x):
    """(x, r) after x += omega T^-1 r on the systems first, first + step, ...; r holds d there.  The inputs are not changed."""
    lo, minv, cp = fac
    r, x = r.copy(), x.copy()
    L, M, C, R, X = (by_system(v, W, direction)[first::step] for v in (lo, minv, cp, r, x))
    n = R.shape[1]
    if R.shape[0] == 0:
        return x, r
    R[:, 0] = R[:, 0] * M[:, 0]
    for j in range(1, n):
        R[:, j] = (R[:, j] - L[:, j] * R[:, j - 1]) * M[:, j]
    e = R[:, n - 1].copy()
    X[:, n - 1] = X[:, n - 1] + omega * e
    for j in range(n - 2, -1, -1):
        e = R[:, j] - C[:, j] * e
        X[:, j] = X[:, j] + omega * e
    return x, r


def half_steps(line_dir, line_order, reverse=False):
    colours = ((0, 2), (1, 2)) if line_order == "zebra" else ((0, 1),)
    out = [(d, first, step) for d in line_dir for (first, step) in colours]
    return out[::-1] if reverse else out


def line_step(A, W, facs, x, b, line_dir="xy", line_order="zebra", omega=1.0, reverse=False, steps=1):
    """`steps` smoothing steps from x; facs: {"x": triple, "y": triple} for the directions used."""
    x = np.ascontiguousarray(x, dtype=float).reshape(-1).copy()
    for _ in range(steps):
        for d, first, step in half_steps(line_dir, line_order, reverse):
            r, _ = K.residual(A, x, b)
            x, _ = solve(facs[d], W, d, first, step, r, omega, x)
    return x


def square_stride(n):
    W = int(round(np.sqrt(n)))
    assert W * W == n, "give the line strides of non-square grids explicitly"
    return W


class LineCycle:
    """V-, W- and F-cycles with `steps` line relaxation steps before and (reversed) after the coarse correction.  A: the
    operators of all levels, P / R: the transfers, coarse(rc) -> the coarsest-level solution, strides: the line stride of every
    smoothed level (None: square grids)."""

    def __init__(self, A, P, R, coarse, strides=None, line_dir="xy", line_order="zebra", omega=1.0):
        self.A = [K.as_csr(a) for a in A]
        self.P = [K.as_csr(p) for p in P]
        self.R = [K.as_csr(r) for r in R]
        self.coarse = coarse
        self.W = [square_stride(a.shape[0]) for a in self.A[:-1]] if strides is None else list(strides)
        self.line_dir, self.line_order, self.omega = line_dir, line_order, omega
        self.facs = []
        for a, W in zip(self.A[:-1], self.W):
            f = {}
            for d in line_dir:
                f[d], flags = factor(a, W, d)
                assert flags == 0, (a.shape, d, flags)
            self.facs.append(f)

    @classmethod
    def galerkin(cls, A, hierarchy, **kw):
        """R = P^T, A_(l+1) = (R A) P, the coarsest level solved by a sparse LU."""
        from scipy.sparse.linalg import splu
        As = [K.as_csr(A)]
        Ps = [K.as_csr(sp.csr_matrix(p)) for p in hierarchy]
        Rs = [K.as_csr(p.T.tocsr()) for p in Ps]
        for l in range(len(Ps)):
            As.append(K.as_csr(sp.csr_matrix((Rs[l] @ As[l]) @ Ps[l])))
        lu = splu(sp.csc_matrix(As[-1]))
        return cls(As, Ps, Rs, lu.solve, **kw)

    def smooth(self, l, x, b, steps, reverse=False):
        return line_step(self.A[l], self.W[l], self.facs[l], x, b, self.line_dir, self.line_order, self.omega, reverse, steps)

    def cycle(self, x, b, steps=1, l=0, shape="V"):
        b = np.ascontiguousarray(b, dtype=float).reshape(-1)
        x = self.smooth(l, x, b, steps)
        r, _ = K.residual(self.A[l], x, b)
        rc = K.matvec(self.R[l], r)
        if l + 1 == len(self.P):
            ec = self.coarse(rc)
        else:
            ec = np.zeros_like(rc)
            for sub in CHILDREN[shape]:
                ec = self.cycle(ec, rc, steps, l + 1, sub)
        x = K.spmv(self.P[l], ec, x, 1.0, 1.0)
        return self.smooth(l, x, b, steps, reverse=True)


def history(ref, A, rhs, cycles, **kw):
    """||b - A x|| before each of `cycles` cycles from a zero guess and after the last one, and the final iterate."""
    A = K.as_csr(A)
    b = np.asarray(rhs, dtype=float).ravel()
    x = np.zeros(A.shape[0])
    out = [np.sqrt(K.residual(A, x, b)[1])]
    for _ in range(cycles):
        x = ref.cycle(x, b, **kw)
        out.append(np.sqrt(K.residual(A, x, b)[1]))
    return np.array(out), x
