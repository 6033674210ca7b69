"""CPU restatement of line relaxation with banded line systems (half-bandwidth p = 2, 3) -- TEST INFRASTRUCTURE ONLY.

Plain NumPy, vectorised across the systems of a direction like line_ref.py, written from the definition.  A level has n rows
and a line stride W.  Direction "x": system = storage line, its matrix B the entries of A at column - row = m, |m| <= p,
that stay inside the line (one that leaves it belongs to no system; a non-zero one sets COUPLED).  Direction "y": system =
grid column, the entries at column - row = c W, |c| <= p.  A missing entry is 0, every other entry of A is off-line
coupling and only enters through the residual.

The order of the arithmetic (every product and every difference rounds on its own; the kernels follow it bit for bit).
Rows before the first and behind the last of a system count as ZERO rows -- all entries, minv, d and e are 0 there -- so
every row runs the same p steps.  With j the place of a row in its system:

    factor   w_m = B_(j,j+m), m = -p .. p
             for t = p, p - 1, .., 1      (the rows j - p .. j - 1 in that order)
                 l_(j,t) = w_(-t) * minv_(j-t)
                 for q = 1 .. p:  w_(-t+q) = w_(-t+q) - l_(j,t) * u_(j-t,q)
             u_(j,q) = w_q, q = 0 .. p;   minv_j = 1.0 / u_(j,0)             (PIVOT: u_(j,0) zero or not finite)
    forward  s = r_j;  for t = p, .., 1:  s = s - l_(j,t) * d_(j-t);   d_j = s                        (d overwrites r)
    backward s = d_j;  for q = p, .., 1:  s = s - u_(j,q) * e_(j+q);   e_j = s * minv_j;   x_j = x_j + omega * e_j

The farthest row is subtracted first.  The factors are 2 p + 1 planes of n doubles indexed by row, fac[t - 1] = l_(.,t),
fac[p] = minv, fac[p + q] = u_(.,q): the layout of lmg_line_factor_banded.

LineBandCycle runs the cycles of line_ref.LineCycle with a half-bandwidth per level and direction (1: line_ref's own
tridiagonal factor and solve).  stand_in() is the CPU stand-in of the ops module for host-logic tests.
"""
import numpy as np
import scipy.sparse as sp
import torch

import cpu_ops_shim
import line_ref as LR
from learnmultigrid_amd import problems as P
from oracle import kernels as K
from support import to_numpy as _np, to_scipy as _sp

COUPLED, PIVOT = LR.COUPLED, LR.PIVOT
by_system = LR.by_system


def bands(A, W, direction, p):
    """(B, flags): B[(m + p), row] = the entry of the row's system at distance m, m = -p .. p; flags has COUPLED set if, in
    direction x, a stored non-zero entry with |column - row| <= p leaves its line."""
    A = K.as_csr(A)
    n = A.shape[0]
    assert n % W == 0 and p >= 1
    s = 1 if direction == "x" else W
    coo = A.tocoo()
    off = coo.col.astype(np.int64) - coo.row
    B = np.zeros((2 * p + 1, n))
    for m in range(-p, p + 1):
        hit = off == m * s
        B[m + p, coo.row[hit]] = coo.data[hit]
    flags = 0
    if direction == "x":
        col = np.arange(n) % W
        for m in range(-p, p + 1):
            out = (col + m < 0) | (col + m >= W)
            if m != 0 and np.any(B[m + p, out] != 0):
                flags |= COUPLED
            if m != 0:
                B[m + p, out] = 0.0
    return B, flags


def factor(A, W, direction, p):
    """(fac, flags): fac (2 p + 1, n), the planes of the module docstring; PIVOT set if a pivot is zero or not finite."""
    B, flags = bands(A, W, direction, p)
    fac = np.empty_like(B)
    Bs = [by_system(B[k], W, direction) for k in range(2 * p + 1)]
    Fs = [by_system(fac[k], W, direction) for k in range(2 * p + 1)]
    nsys, L = Bs[0].shape
    up = [[np.zeros(nsys) for _ in range(p)] for _ in range(p)]       # up[t - 1][q - 1] = u_(j-t,q)
    mv = [np.zeros(nsys) for _ in range(p)]                           # mv[t - 1] = minv_(j-t)
    bad = False
    with np.errstate(all="ignore"):
        for j in range(L):
            w = [Bs[k][:, j].copy() for k in range(2 * p + 1)]
            for t in range(p, 0, -1):
                lt = w[p - t] * mv[t - 1]
                for q in range(1, p + 1):
                    w[p - t + q] = w[p - t + q] - lt * up[t - 1][q - 1]
                Fs[t - 1][:, j] = lt
            bad |= bool(np.any((w[p] == 0) | ~np.isfinite(w[p])))
            minv = 1.0 / w[p]
            Fs[p][:, j] = minv
            for q in range(1, p + 1):
                Fs[p + q][:, j] = w[p + q]
            up = [[w[p + q] for q in range(1, p + 1)]] + up[:-1]
            mv = [minv] + mv[:-1]
    return fac, flags | (PIVOT if bad else 0)


def solve(fac, W, direction, p, first, step, r, omega, x):
    """(x, r) after x += omega (L U)^-1 r on the systems first, first + step, ...; r holds d there.  Inputs unchanged."""
    fac = np.asarray(fac).reshape(2 * p + 1, -1)
    r, x = r.copy(), x.copy()
    Fs = [by_system(fac[k], W, direction)[first::step] for k in range(2 * p + 1)]
    R, X = (by_system(v, W, direction)[first::step] for v in (r, x))
    nsys, L = R.shape
    if nsys == 0:
        return x, r
    with np.errstate(all="ignore"):
        d = [np.zeros(nsys) for _ in range(p)]                        # d[t - 1] = d_(j-t)
        for j in range(L):
            s = R[:, j].copy()
            for t in range(p, 0, -1):
                s = s - Fs[t - 1][:, j] * d[t - 1]
            d = [s] + d[:-1]
            R[:, j] = s
        e = [np.zeros(nsys) for _ in range(p)]                        # e[q - 1] = e_(j+q)
        for j in range(L - 1, -1, -1):
            s = R[:, j].copy()
            for q in range(p, 0, -1):
                s = s - Fs[p + q][:, j] * e[q - 1]
            s = s * Fs[p][:, j]
            e = [s] + e[:-1]
            X[:, j] = X[:, j] + omega * s
    return x, r


def dense_band(B, W, direction, p, k):
    """The matrix of system k from bands()' B, in scipy.linalg.solve_banded's (p, p) storage."""
    Bs = [by_system(B[m], W, direction)[k] for m in range(2 * p + 1)]
    L = Bs[0].size
    ab = np.zeros((2 * p + 1, L))
    for m in range(-p, p + 1):                                        # ab[p + i - j, j] = a_ij with j = i + m
        for i in range(L):
            if 0 <= i + m < L:
                ab[p - m, i + m] = Bs[m + p][i]
    return ab


def _band_of(b, d):
    return int(b[d]) if isinstance(b, dict) else int(b)


class LineBandCycle(LR.LineCycle):
    """line_ref.LineCycle with a half-bandwidth per smoothed level: bands[l] an int or {"x": p, "y": p}.  p = 1 runs
    line_ref's factor and solve, p > 1 this module's."""

    def __init__(self, A, P, R, coarse, bands, strides=None, line_dir="xy", line_order="zebra", omega=1.0):
        self.A = [K.as_csr(a) for a in A]
        self.P = [K.as_csr(p) for p in P]
        self.R = [K.as_csr(r) for r in R]
        self.coarse = coarse
        self.W = [LR.square_stride(a.shape[0]) for a in self.A[:-1]] if strides is None else list(strides)
        self.line_dir, self.line_order, self.omega = line_dir, line_order, omega
        self.bands = [{d: _band_of(b, d) for d in line_dir} for b in bands]
        assert len(self.bands) == len(self.A) - 1
        self.facs = []
        for a, W, b in zip(self.A[:-1], self.W, self.bands):
            f = {}
            for d in line_dir:
                f[d], flags = LR.factor(a, W, d) if b[d] == 1 else factor(a, W, d, b[d])
                assert flags == 0, (a.shape, d, b[d], flags)
            self.facs.append(f)

    def smooth(self, l, x, b, steps, reverse=False):
        x = np.ascontiguousarray(x, dtype=float).reshape(-1).copy()
        W, p = self.W[l], self.bands[l]
        for _ in range(steps):
            for d, first, step in LR.half_steps(self.line_dir, self.line_order, reverse):
                r, _ = K.residual(self.A[l], x, b)
                if p[d] == 1:
                    x, _ = LR.solve(self.facs[l][d], W, d, first, step, r, self.omega, x)
                else:
                    x, _ = solve(self.facs[l][d], W, d, p[d], first, step, r, self.omega, x)
        return x


history = LR.history


# ---- the operators and transfers the tests of the banded lines share ---------------------------------------------------------
def window_operator(Wg, Hg, p, seed, dominant=True):
    """An operator on the Wg x Hg grid with an entry on every offset of the (2p+1)^2 window that stays inside the grid
    (none across a line end), all values distinct; dominant: the diagonal exceeds the sum of the rest of its row."""
    rng = np.random.default_rng(seed)
    n = Wg * Hg
    y, x = np.divmod(np.arange(n), Wg)
    rows, cols = [], []
    for c in range(-p, p + 1):
        for d in range(-p, p + 1):
            ok = (x + d >= 0) & (x + d < Wg) & (y + c >= 0) & (y + c < Hg)
            rows.append(np.flatnonzero(ok))
            cols.append(np.flatnonzero(ok) + c * Wg + d)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.permutation(rows.size) / rows.size - 0.5 + 1e-3         # distinct, none zero
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n)).tolil()
    if dominant:
        A.setdiag(np.asarray(abs(sp.csr_matrix(A)).sum(axis=1)).ravel() + 1.0 + rng.random(n))
    return K.as_csr(sp.csr_matrix(A))


def transfers(kind, side=65, levels=4):
    out = []
    for l, s in enumerate(P.level_sizes(side, levels)[:-1]):
        q = P.pseudo_l2_interpolator_1d(s)
        base = sp.kron(q, q, format="csr")
        out.append(P.learned_like(base, seed=5 + l) if kind == "learned_like" else base)
    return out


def symmetrised(A):
    """Boundary rows and columns eliminated: the interior block next to an identity (tests/block_cg_ref.problem)."""
    A = sp.csr_matrix(A)
    bnd = np.diff(A.indptr) == 1
    keep = sp.diags((~bnd).astype(float))
    S = sp.csr_matrix(keep @ A @ keep + sp.diags(bnd.astype(float)))
    assert abs(S - S.T).max() <= 1e-12 * abs(S).max()
    return K.as_csr(S)


# ---- the CPU stand-ins of ops.line_factor_banded_flags / line_factor_banded / line_solve_banded ---------------------------
def line_factor_banded_flags(A, W, dir, band):
    fac, flags = factor(_sp(A), int(W), dir, int(band))
    return torch.from_numpy(fac.reshape(-1)), flags


def line_factor_banded(A, W, dir, band):
    fac, flags = line_factor_banded_flags(A, W, dir, band)
    if flags & COUPLED:
        raise ValueError("a non-zero entry couples two x-lines (an entry across the end of a line)")
    if flags & PIVOT:
        raise ValueError("a zero or non-finite pivot in the %s-line systems" % dir)
    return fac


def line_solve_banded(W, dir, band, first, step, fac, r, omega, x):
    xn, rn = solve(_np(fac), int(W), dir, int(band), int(first), int(step), _np(r), float(omega), _np(x))
    _np(x)[:] = xn
    _np(r)[:] = rn


def stand_in():
    """cpu_ops_shim.recording_line() with the banded stand-ins, which record ("factor_banded", n, W, dir, band) and
    ("solve_banded", n, dir, band, first, step, omega) in ns.calls."""
    ns = cpu_ops_shim.recording_line()

    def rec_line_factor_banded(A, W, dir, band):
        ns.calls.append(("factor_banded", A.shape[0], int(W), dir, int(band)))
        return line_factor_banded(A, W, dir, band)

    def rec_line_solve_banded(W, dir, band, first, step, fac, r, omega, x):
        line_solve_banded(W, dir, band, first, step, fac, r, omega, x)
        ns.calls.append(("solve_banded", x.numel(), dir, int(band), int(first), int(step), float(omega)))

    ns.line_factor_banded_flags = line_factor_banded_flags
    ns.line_factor_banded, ns.line_solve_banded = rec_line_factor_banded, rec_line_solve_banded
    return ns
