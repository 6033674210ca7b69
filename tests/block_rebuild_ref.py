"""TEST-ONLY helpers of the block-cycle-after-rebuild tests (tests/test_block_rebuild_*.py): the second set of values for the
block tests' own problem, the oracle histories on either set, and the values of a lagged preconditioner.

The problem is the one of tests/test_block_cycle_gpu.py: jittered_poisson_2d(32, seed=42), n = 1089, with the learned-like
pseudo-L2 transfers 1089 -> 289 -> 81, V(2, 2) weighted Jacobi at omega = 0.8, 8 cycles, the columns of that file (the
problem's own right-hand side, then default_rng(5) normal columns).  A2 is the same mesh with a log-normal element coefficient
(coeff_sigma = 0.5, coeff_seed = 45): the same sparsity pattern, other values on every level."""
import functools

import numpy as np
import scipy.sparse as sp

import block_cg_ref as C
from cycle_shapes_ref import ShapeCycle
from learnmultigrid_amd import problems as P
from oracle import kernels as K
from oracle.vcycle_ref import HoistedVCycle

RTOL = 1e-10                     # the project's tolerance for histories
CYCLES = 8
LEVELS, STEPS, OMEGA = 3, 2, 0.8
NCOLS = 3
LAG = 0.1                        # the lagged preconditioner is built on A + LAG * diag(A)


@functools.lru_cache(maxsize=None)
def problem(levels=LEVELS):
    """(A1, A2, hier, B): both operators as CSR on one pattern, the transfers, and 11 right-hand sides (n, 11), read-only."""
    A1, rhs = P.jittered_poisson_2d(32, seed=42)
    A2 = P.jittered_poisson_2d(32, seed=42, coeff_sigma=0.5, coeff_seed=45)[0]
    A1, A2 = K.as_csr(sp.csr_matrix(A1)), K.as_csr(sp.csr_matrix(A2))
    B = np.column_stack([rhs.ravel(), np.random.default_rng(5).standard_normal((A1.shape[0], 10))])
    B.setflags(write=False)
    return A1, A2, C.learned_like_hierarchy(C.SIDE, levels), B


def histories(A, hier, B, shape="V", cycles=CYCLES):
    """Per column of B: ||b - A x|| before each of `cycles` cycles of the oracle and after the last (cycles + 1 rows), and
    the last iterate."""
    ref = HoistedVCycle(A, hier) if shape == "V" else ShapeCycle(A, hier, shape)
    hist, X = np.empty((cycles + 1, B.shape[1])), np.empty(B.shape)
    for j in range(B.shape[1]):
        x = np.zeros(A.shape[0])
        for it in range(cycles):
            hist[it, j] = np.linalg.norm(B[:, j] - A @ x)
            x = ref.cycle(x, B[:, j], "Jacobi", STEPS, OMEGA)
        hist[cycles, j] = np.linalg.norm(B[:, j] - A @ x)
        X[:, j] = x
    return hist, X


@functools.lru_cache(maxsize=None)
def reference(which, levels=LEVELS, shape="V", cycles=CYCLES):
    """histories() of the first NCOLS columns on A1 (which = 1) or A2 (which = 2), computed once and read-only."""
    A1, A2, hier, B = problem(levels)
    hist, X = histories(A1 if which == 1 else A2, hier, B[:, :NCOLS], shape, cycles)
    hist.setflags(write=False)
    X.setflags(write=False)
    return hist, X


def lagged_values(A):
    """The values of A + LAG * diag(A) in the storage order of A (canonical CSR with a stored diagonal in every row): the
    same pattern, and symmetric where A is."""
    A = sp.csr_matrix(A)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    on = A.indices == rows
    assert on.sum() == A.shape[0]
    vals = A.data.copy()
    vals[on] *= 1.0 + LAG
    return vals


def with_values(A, vals):
    return K.as_csr(sp.csr_matrix((vals, A.indices, A.indptr), shape=A.shape))


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)


def close_x(got, want):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=RTOL * np.abs(want).max())
