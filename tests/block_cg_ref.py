"""TEST-ONLY helpers of the block conjugate-gradient tests (tests/test_block_cg_*.py): the test problem, the textbook
recurrence in NumPy (pcg_ref), and NumPy stand-ins of the block ops -- the sweeps BlockCycle needs and the three CG
kernels -- for cpu_ops_shim.namespace(**replace), so that krylov.block_pcg runs on CPU tensors.

The problem: jittered_poisson_2d(32, seed=42) with the Dirichlet couplings eliminated (A = A^T), the 3-level learned-like
pseudo-L2 hierarchy 1089 -> 289 -> 81 with a dense coarse solve, columns = the problem's own right-hand side and
default_rng(5) normal columns, V(2, 2) weighted Jacobi at omega = 0.8 as the preconditioner."""
import functools

import numpy as np
import scipy.sparse as sp

from cycle_shapes_ref import ShapeCycle
from learnmultigrid_amd import problems as P
from oracle import kernels as K
from oracle.vcycle_ref import HoistedVCycle
from support import to_numpy as _np, to_scipy as _sp

WIDTHS = (2, 4, 8)
SIDE, LEVELS, STEPS, OMEGA = 33, 3, 2, 0.8
MMAX = 11
ITERATIONS = 8                   # of the history checks: every column is at 2e-9 .. 3e-10 of its start, no floor in sight
RTOL = 1e-10                     # the project's tolerance for histories (four orders above what summation order moves)


def learned_like_hierarchy(side=SIDE, levels=LEVELS, seed=43):
    hier = []
    for l, s in enumerate(P.level_sizes(side, levels)[:-1]):
        base = sp.kron(P.pseudo_l2_interpolator_1d(s), P.pseudo_l2_interpolator_1d(s)).tocsr()
        hier.append(P.learned_like(base, seed + l))
    return hier


@functools.lru_cache(maxsize=None)
def problem():
    """(A, hier, B): the symmetric operator, the transfers, and the MMAX right-hand sides (n, MMAX), read-only."""
    A, rhs = P.jittered_poisson_2d(SIDE - 1, seed=42)
    A = sp.csr_matrix(A)
    idx = np.arange(SIDE * SIDE)
    inter = ((idx % SIDE) > 0) & ((idx % SIDE) < SIDE - 1) & ((idx // SIDE) > 0) & ((idx // SIDE) < SIDE - 1)
    keep = sp.diags(inter.astype(float))
    A = sp.csr_matrix(keep @ A @ keep + sp.diags((~inter).astype(float)))
    assert abs(A - A.T).max() <= 1e-12 * abs(A).max()
    A = K.as_csr(A)
    B = np.column_stack([rhs.ravel(), np.random.default_rng(5).standard_normal((A.shape[0], MMAX - 1))])
    B.setflags(write=False)
    return A, learned_like_hierarchy(), B


@functools.lru_cache(maxsize=None)
def cycle_operator(shape="V"):
    """M(v): one `shape` cycle of the oracle on the right-hand side v from a zero guess -- the preconditioner."""
    A, hier, _ = problem()
    ref = HoistedVCycle(A, hier) if shape == "V" else ShapeCycle(A, hier, shape)
    return lambda v: ref.cycle(np.zeros(A.shape[0]), v, "Jacobi", STEPS, OMEGA)


def dot_numpy(x, y):
    return float(np.dot(x, y))


def dot_reversed(x, y):
    """The same products summed one by one from the last to the first: another order than NumPy's pairwise blocks."""
    s = 0.0
    for v in (x * y)[::-1].tolist():
        s += v
    return s


def pcg_ref(A, b, M, iterations, x0=None, dot=dot_numpy):
    """The textbook preconditioned CG recurrence, `iterations` steps whatever the residual does (M None: plain CG).
    Returns (track, Xs): track[0] = ||b - A x0||, track[i] = sqrt(r_i . r_i) of the recurrence; Xs[i] the iterate after i
    steps."""
    b = np.asarray(b, dtype=float).reshape(-1)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=float).reshape(-1)
    r = b - A @ x
    track, Xs = [float(np.linalg.norm(r))], [x.copy()]
    z = r.copy() if M is None else M(r)
    p = z.copy()
    rz = dot(r, z)
    for _ in range(iterations):
        Ap = A @ p
        pAp = dot(p, Ap)
        alpha = rz / pAp if pAp != 0.0 else 0.0
        x = alpha * p + x
        r = -alpha * Ap + r
        rr = dot(r, r)
        track.append(float(np.sqrt(rr)))
        Xs.append(x.copy())
        z = r if M is None else M(r)
        rz_new = rr if M is None else dot(r, z)
        beta = rz_new / rz if rz != 0.0 else 0.0
        rz = rz_new
        p = z + beta * p
    return np.array(track), np.array(Xs)


@functools.lru_cache(maxsize=None)
def reference(shape="V", iterations=14, ncols=MMAX):
    """pcg_ref of the first ncols columns from a zero guess (shape None: no preconditioner): (track, Xs) with the column
    as the last axis, computed once and read-only."""
    A, _, B = problem()
    M = None if shape is None else cycle_operator(shape)
    runs = [pcg_ref(A, B[:, j], M, iterations) for j in range(ncols)]
    track, Xs = np.stack([t for t, _ in runs], axis=1), np.stack([x for _, x in runs], axis=2)
    track.setflags(write=False)
    Xs.setflags(write=False)
    return track, Xs


def first_pass(track, error):
    """Per column the first iteration (row of track, >= 1) whose recurrence norm is <= error; 0 where row 0 already is."""
    return [0 if track[0, j] <= error else int(np.flatnonzero(track[1:, j] <= error)[0]) + 1 for j in range(track.shape[1])]


# ---- NumPy stand-ins of the block ops ----------------------------------------------------------------------------------------
def block_residual_norm2(S, X, B, R, partials, norm2):
    r = _np(B) - _sp(S) @ _np(X)
    if R is not None:
        _np(R)[:] = r
    if norm2 is not None:
        _np(norm2)[:r.shape[1]] = (r * r).sum(axis=0)


def block_jacobi(S, X, B, omega, Out):
    A = _sp(S)
    d = A.diagonal()[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        _np(Out)[:] = np.where(d != 0, _np(X) + omega * ((1.0 / d) * (_np(B) - A @ _np(X))), _np(X))


def block_spmv(S, X, Y, alpha=1.0, beta=0.0):
    _np(Y)[:] = alpha * (_sp(S) @ _np(X)) + (beta * _np(Y) if beta != 0.0 else 0.0)


def dense_gemv_block(M, X, Y):
    _np(Y)[:] = _np(M) @ _np(X)


def block_dot(X, Y, partials, out):
    k = X.shape[1]
    _np(out)[:k] = [float(np.dot(_np(X)[:, j], _np(Y)[:, j])) for j in range(k)]


def block_cg_step(rz, pAp, tol2, mask, P, AP, X, R, partials, rr):
    k = X.shape[1]
    for j in range(k):
        if _np(mask)[j] != 0.0:
            alpha = _np(rz)[j] / _np(pAp)[j] if _np(pAp)[j] != 0.0 else 0.0
            _np(X)[:, j] = alpha * _np(P)[:, j] + _np(X)[:, j]
            _np(R)[:, j] = -alpha * _np(AP)[:, j] + _np(R)[:, j]
        _np(rr)[j] = float(np.dot(_np(R)[:, j], _np(R)[:, j]))
        _np(mask)[j] = 1.0 if _np(mask)[j] != 0.0 and _np(rr)[j] > _np(tol2)[j] else 0.0


def block_cg_direction(rz_new, rz_old, mask, Z, P):
    assert rz_new.data_ptr() != rz_old.data_ptr() and Z.data_ptr() != P.data_ptr()
    for j in range(P.shape[1]):
        if _np(mask)[j] != 0.0:
            beta = _np(rz_new)[j] / _np(rz_old)[j]
            # (beta == 0 stores Z and does not read P, like the kernel: axpby's beta == 0 case)
            _np(P)[:, j] = _np(Z)[:, j] if beta == 0.0 else _np(Z)[:, j] + beta * _np(P)[:, j]


def block_namespace(shim, **replace):
    """shim.namespace() with the block ops on (n, k) CPU tensors (a "twin" is the matrix itself) and `replace` on top."""
    ops = dict(BLOCK_WIDTHS=WIDTHS, block_twin=lambda A: A, block_partials_count=lambda n, k: (n // 256 + 1) * k,
               block_dot_partials_count=lambda n, k: 1024 * k, block_residual_norm2=block_residual_norm2,
               block_jacobi=block_jacobi, block_spmv=block_spmv, dense_gemv_block=dense_gemv_block, block_dot=block_dot,
               block_cg_step=block_cg_step, block_cg_direction=block_cg_direction)
    ops.update(replace)
    return shim.namespace(**ops)
