"""TEST-ONLY helpers of the block GMRES tests (tests/test_block_gmres_*.py): the test problem, the reference histories
(krylov_ref.fgmres_ref column by column with the oracle's cycle as M), the tolerance, and NumPy stand-ins of the three block
Gram-Schmidt ops for cpu_ops_shim.namespace(**replace), so that krylov.block_fgmres runs on CPU tensors.  The block sweep
stand-ins come from block_cg_ref.

The problem: jittered_poisson_2d(32, seed=42) AS IT COMES -- n = 1089, odd, Dirichlet rows kept as identity rows with the
columns left alone, so A != A^T --, the 3-level learned-like hierarchy 1089 -> 289 -> 81 of block_cg_ref with a dense coarse
solve, columns = the problem's own right-hand side and default_rng(5) normal columns, 11 in all, and a copy scaled by
10^(-j/2) for the stopping tests: with one threshold the columns then stop at different steps.

The tolerance.  A GMRES history cannot be compared at a fixed relative tolerance beyond its first restart: the recomputed
true residual sits on an absolute floor of about 1e-16 |r_0|, and what is left of it is what the next cycle starts from.
So histories are compared with |got - want| <= RTOL * want + ATOL * track[0, j]: RTOL is the project's figure, ATOL is
100 times what right-hand sides perturbed by 4e-16 relative (every entry, random signs) move the NumPy reference over 10
iterations of GMRES(4), relative to track[0].  Measured with the V cycle, the F cycle and no preconditioner: the ten normal
columns move by <= 3e-16, the problem's own right-hand side (column 0, whose first step gains least) by 2.0e-15 .. 2.6e-15
depending on the signs drawn; MOVE is that figure rounded up, and test_block_gmres_cpu.py asserts the measurement.  The factor 100 covers the difference
between a perturbation of one input and the accumulated reordering of every sum on the device.  Solutions use the same
two-term bound with |x|_max in place of track[0]."""
import functools

import numpy as np
import scipy.sparse as sp

import block_cg_ref as C
from cycle_shapes_ref import ShapeCycle
from krylov_ref import fgmres_ref
from learnmultigrid_amd import problems as P
from oracle import kernels as K
from oracle.vcycle_ref import HoistedVCycle
from support import to_numpy as _np

WIDTHS = C.WIDTHS
STEPS, OMEGA = C.STEPS, C.OMEGA
MMAX = 11
RESTART, ITERATIONS = 4, 10      # of the history checks: two full cycles and half of a third
RTOL = 1e-10                     # the project's tolerance for histories
MOVE = 3e-15                 # what a 4e-16 perturbation of b moves a history, relative to track[0] (asserted on the CPU)
ATOL = 100 * MOVE


def perturbed(b, seed):
    """b with every entry moved by 4e-16 relative, signs from default_rng(seed)."""
    return b * (1.0 + 4e-16 * np.random.default_rng(seed).choice((-1.0, 1.0), b.size))
STOP_ERROR = 1e-6                # of the stopping tests, on the scaled right-hand sides
STOP_COUNTS = [6, 7, 7, 6, 6, 5, 5, 4, 4, 3, 3]


@functools.lru_cache(maxsize=None)
def problem():
    """(A, hier, B, Bs): the unsymmetric operator, the transfers, the MMAX right-hand sides (n, MMAX) and their scaled
    copy B[:, j] * 10^(-j/2), read-only."""
    A, rhs = P.jittered_poisson_2d(C.SIDE - 1, seed=42)
    A = K.as_csr(sp.csr_matrix(A))
    assert A.shape[0] == 1089 and abs(A - A.T).max() > 0.1 * abs(A).max()          # not symmetric, and not by rounding
    B = np.column_stack([rhs.ravel(), np.random.default_rng(5).standard_normal((A.shape[0], MMAX - 1))])
    Bs = B * 10.0 ** (-np.arange(MMAX) / 2.0)
    B.setflags(write=False)
    Bs.setflags(write=False)
    return A, C.learned_like_hierarchy(), B, Bs


@functools.lru_cache(maxsize=None)
def cycle_operator(shape="V"):
    """M(v): one `shape` cycle of the oracle on the right-hand side v from a zero guess -- the preconditioner; None: none."""
    if shape is None:
        return None
    A, hier, _, _ = problem()
    ref = HoistedVCycle(A, hier) if shape == "V" else ShapeCycle(A, hier, shape)
    return lambda v: ref.cycle(np.zeros(A.shape[0]), v, "Jacobi", STEPS, OMEGA)


def pad_tracks(tracks):
    """Histories of different lengths as the columns of one array, NaN behind each."""
    out = np.full((max(len(t) for t in tracks), len(tracks)), np.nan)
    for j, t in enumerate(tracks):
        out[:len(t), j] = t
    return out


@functools.lru_cache(maxsize=None)
def reference(shape="V", scaled=False, max_iterations=ITERATIONS, error=0.0, restart=RESTART):
    """fgmres_ref of every column from a zero guess: (X (n, MMAX), track (rows, MMAX) NaN-padded, iterations), computed
    once and read-only."""
    A, _, B, Bs = problem()
    rhs = Bs if scaled else B
    runs = [fgmres_ref(A, rhs[:, j], cycle_operator(shape), restart=restart, max_iterations=max_iterations, error=error)
            for j in range(MMAX)]
    X, track = np.column_stack([r[0] for r in runs]), pad_tracks([r[1] for r in runs])
    X.setflags(write=False)
    track.setflags(write=False)
    return X, track, [r[2] for r in runs]


def close(got, want):
    """Histories (rows, columns): the two-term bound column by column, NaN where and only where the reference has it."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    bound = RTOL * np.abs(want) + ATOL * want[0][None, :]
    err = np.abs(got - want)
    assert (err[ok] <= bound[ok]).all(), "largest |got - want| / bound = %.3g" % (err[ok] / bound[ok]).max()


def close_x(got, want):
    """Solutions (n, columns): the same bound with |x|_max of the column in place of track[0]."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bound = RTOL * np.abs(want) + ATOL * np.abs(want).max(axis=0)[None, :]
    err = np.abs(got - want)
    assert (err <= bound).all(), "largest |got - want| / bound = %.3g" % (err / np.maximum(bound, 1e-300)).max()


# ---- NumPy stand-ins of the block Gram-Schmidt ops ----------------------------------------------------------------------------
def block_multi_partials_count(n, k, nb):
    return 1024 * k * max(int(nb), 1)


def block_multi_dot(V, nb, W, partials, out):
    n, k = W.shape
    assert V.dim() == 3 and V.is_contiguous() and tuple(V.shape[1:]) == (n, k) and 0 <= nb <= V.shape[0]
    Vn, Wn, on = _np(V), _np(W), _np(out)
    for i in range(nb):
        for j in range(k):
            on[i * k + j] = float(Vn[i, :, j] @ Wn[:, j])


def block_multi_axpy(V, counts, coef, W, partials=None, norm2=None, subtract=True):
    n, k = W.shape
    assert V.dim() == 3 and V.is_contiguous() and tuple(V.shape[1:]) == (n, k) and len(counts) == k
    assert all(0 <= c <= V.shape[0] for c in counts) and V.data_ptr() != W.data_ptr()
    Vn, Wn, c = _np(V), _np(W), _np(coef).copy()          # (coef may be a view of the buffer norm2 lives in)
    for j in range(k):
        w = Wn[:, j].copy()
        for i in range(counts[j]):
            w = w - c[i * k + j] * Vn[i, :, j] if subtract else w + c[i * k + j] * Vn[i, :, j]
        if counts[j]:
            Wn[:, j] = w
    if norm2 is not None:
        assert partials is not None
        _np(norm2)[:k] = [float(Wn[:, j] @ Wn[:, j]) for j in range(k)]


def block_scale(scale, W):
    assert len(scale) == W.shape[1]
    Wn = _np(W)
    for j, s in enumerate(scale):
        Wn[:, j] = 0.0 if s == 0.0 else s * Wn[:, j]


def block_namespace(shim, **replace):
    """block_cg_ref.block_namespace with the three Gram-Schmidt ops on top, and `replace` on top of those."""
    ops = dict(block_multi_partials_count=block_multi_partials_count, block_multi_dot=block_multi_dot,
               block_multi_axpy=block_multi_axpy, block_scale=block_scale)
    ops.update(replace)
    return C.block_namespace(shim, **ops)
