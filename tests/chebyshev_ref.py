"""CPU restatement of the Chebyshev polynomial smoother and of the cycles that use it -- TEST INFRASTRUCTURE ONLY.

Plain NumPy over the oracle's row sums (oracle.kernels.residual gives b - rsum with rsum in storage order), written from the
definition: on a level with bounds [lmin, lmax] for D^-1 A,
    theta = (lmax + lmin) / 2,  delta = (lmax - lmin) / 2,  sigma = theta / delta,  rho_0 = 1 / sigma,
    k = 0:  a_0 = 0, c_0 = 1 / theta;     k >= 1:  rho_k = 1 / (2 sigma - rho_(k-1)), a_k = rho_k rho_(k-1), c_k = 2 rho_k / delta,
and per row and sweep, products and sums rounded separately,
    z = rdiag * (b - rsum),   d = a_k * d + c_k * z  (k = 0: d = c_0 * z),   x = x + d.
"""
import numpy as np
import scipy.sparse as sp

from oracle import kernels as K

CHILDREN = {"V": ("V",), "W": ("W", "W"), "F": ("F", "V")}


def coefficients(lmax, ratio, degree):
    lmin = lmax / ratio
    theta = (lmax + lmin) / 2
    delta = (lmax - lmin) / 2
    sigma = theta / delta
    rho = [1 / sigma]
    out = [(0.0, 1 / theta)]
    for k in range(1, degree):
        rho.append(1 / (2 * sigma - rho[k - 1]))
        out.append((rho[k] * rho[k - 1], 2 * rho[k] / delta))
    return out


def _diag_and_abs_sums(A):
    """Per row: the sum of the diagonal entries and the sum of |a_ij|, both in storage order."""
    A = K.as_csr(A)
    n = A.shape[0]
    rp, ci, va = A.indptr, A.indices, A.data
    diag = np.zeros(n)
    asum = np.zeros(n)
    length = np.diff(rp)
    for j in range(int(length.max()) if n else 0):       # entry j of every row that has one: sequential sums per row
        rows = np.nonzero(length > j)[0]
        e = rp[rows] + j
        asum[rows] = asum[rows] + np.abs(va[e])
        on = ci[e] == rows
        diag[rows[on]] = diag[rows[on]] + va[e[on]]
    return diag, asum


def inverse_diagonal(A):
    diag, _ = _diag_and_abs_sums(A)
    out = np.zeros(diag.size)
    np.divide(1.0, diag, out=out, where=diag != 0)
    return out


def gershgorin(A):
    """max_i (sum_j |a_ij|) / |a_ii| over the rows with a non-zero diagonal: a bound of the spectrum of D^-1 A."""
    diag, asum = _diag_and_abs_sums(A)
    ok = diag != 0
    return float(np.max(asum[ok] / np.abs(diag[ok]))) if ok.any() else 0.0


def cheby_step(A, x, b, coef, dinv=None):
    """One smoothing step of degree len(coef) from x; dinv = 1 / diag(A) unless given."""
    A = K.as_csr(A)
    dinv = inverse_diagonal(A) if dinv is None else dinv
    b = np.ascontiguousarray(b, dtype=float).reshape(-1)
    x = np.ascontiguousarray(x, dtype=float).reshape(-1).copy()
    d = None
    for k, (a, c) in enumerate(coef):
        r, _ = K.residual(A, x, b)
        z = dinv * r
        d = c * z if k == 0 else a * d + c * z
        x = x + d
    return x


class ChebyCycle:
    """V-, W- and F-cycles with one Chebyshev step of degree `degree` before and after the coarse correction.  A: the
    operators of all levels, P / R: the transfers, coarse(rc) -> the coarsest-level solution, lmax: one bound per smoothed
    level (None: its Gershgorin bound)."""

    def __init__(self, A, P, R, coarse, lmax=None, ratio=4.0):
        self.A = [K.as_csr(a) for a in A]
        self.P = [K.as_csr(p) for p in P]
        self.R = [K.as_csr(r) for r in R]
        self.coarse = coarse
        self.dinv = [inverse_diagonal(a) for a in self.A[:-1]]
        self.lmax = [gershgorin(a) for a in self.A[:-1]] if lmax is None else list(lmax)
        self.ratio = ratio

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

    def smooth(self, l, x, b, degree):
        return cheby_step(self.A[l], x, b, coefficients(self.lmax[l], self.ratio, degree), self.dinv[l])

    def cycle(self, x, b, degree=3, l=0, shape="V"):
        b = np.ascontiguousarray(b, dtype=float).reshape(-1)
        x = self.smooth(l, x, b, degree)
        r, _ = K.residual(self.A[l], x, b)
        rc = K.matvec(self.R[l], r)
        if l + 1 == len(self.P):
            ec = self.coarse(rc)
        else:
            ec = np.zeros_like(rc)
            for sub in CHILDREN[shape]:
                ec = self.cycle(ec, rc, degree, l + 1, sub)
        x = K.spmv(self.P[l], ec, x, 1.0, 1.0)
        return self.smooth(l, x, b, degree)


def history(ref, A, rhs, cycles, **kw):
    """||b - A x|| before each of `cycles` cycles from a zero guess, and the final iterate."""
    b = np.asarray(rhs, dtype=float).ravel()
    x = np.zeros(A.shape[0])
    out = []
    for _ in range(cycles):
        out.append(np.sqrt(K.residual(A, x, b)[1]))
        x = ref.cycle(x, b, **kw)
    return np.array(out), x
