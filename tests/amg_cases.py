"""TEST-ONLY: the matrices the classical AMG tests run on (tests/test_amg_cpu.py, tests/test_amg_gpu.py) and the reference
run of a whole hierarchy through the oracle.  Nothing in learnmultigrid_amd imports this file."""
import functools

import numpy as np
import scipy.sparse as sp

import amg_ref as R
from learnmultigrid_amd import problems as P
from oracle import kernels as K, vcycle_ref as V


def renumbered(A, b, seed=7):
    """A symmetric renumbering of (A, b) by a fixed random permutation, rows sorted."""
    p = np.random.default_rng(seed).permutation(A.shape[0])
    M = sp.csr_matrix(A)[p][:, p]
    M.sort_indices()
    return M, b[p]


@functools.lru_cache(maxsize=None)
def problems():
    """name -> (A, rhs): the five 33^2 problems of the convergence and whole-hierarchy tests."""
    out = {"poisson": P.poisson_2d_structured(32), "jittered": P.jittered_poisson_2d(32),
           "anisotropic": P.anisotropic_poisson_2d_structured(32, 0.01, 1.0),
           "variable": P.variable_coeff_poisson_2d_structured(32)}
    out["renumbered"] = renumbered(*out["jittered"])
    return {k: (R.canonical(A), np.asarray(b, dtype=np.float64)) for k, (A, b) in out.items()}


def chain(n):
    """The 1-D operator [-1, 2, -1] on n nodes, no boundary rows."""
    return sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")


def torus(s):
    """The 5-point operator on the periodic s x s grid: every row [-1, -1, 4, -1, -1] in some order, every column count of S
    equal -- only the hash separates the PMIS keys."""
    idx = np.arange(s * s).reshape(s, s)
    rows = np.repeat(idx.ravel(), 5)
    cols = np.stack([idx, np.roll(idx, 1, 0), np.roll(idx, -1, 0), np.roll(idx, 1, 1), np.roll(idx, -1, 1)], -1).ravel()
    vals = np.tile([4.0, -1.0, -1.0, -1.0, -1.0], s * s)
    return sp.csr_matrix((vals, (rows, cols)), shape=(s * s, s * s))


def _without(A, i, j):
    """A without the stored entry (i, j)."""
    C = sp.coo_matrix(A)
    keep = ~((C.row == i) & (C.col == j))
    return sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=A.shape)


@functools.lru_cache(maxsize=None)
def case_matrices():
    """name -> (A, theta): the case matrices of the invariants and of the stage parity, edge shapes included -- the smallest
    at which the kernels can go wrong."""
    pr = problems()
    jit8 = R.canonical(P.jittered_poisson_2d(8)[0])
    empty_row = sp.lil_matrix(chain(9))
    empty_row.rows[4], empty_row.data[4] = [], []
    mixed = sp.lil_matrix(chain(12))
    mixed[5, :] = -mixed[5, :].toarray()                       # one row with a negative diagonal and positive couplings
    uneven = sp.csr_matrix(np.array([[4.0, -1.0, -2.0, 0.5], [-1.0, 3.0, -1.0, -1.0], [-2.0, -1.0, 4.0, -1.0],
                                     [0.5, -1.0, -1.0, 2.5]]))
    cases = {
        "poisson8": (P.poisson_2d_structured(8)[0], 0.25),
        "poisson32": (pr["poisson"][0], 0.25),
        "jittered32": (pr["jittered"][0], 0.25),
        "renumbered32": (pr["renumbered"][0], 0.25),
        "anisotropic32": (pr["anisotropic"][0], 0.25),
        "n1": (sp.csr_matrix(np.array([[2.0]])), 0.25),
        "chain257": (chain(257), 0.25),                        # one lane in the second workgroup
        "empty_row": (sp.csr_matrix(empty_row), 0.25),
        "no_diagonal": (_without(chain(9), 3, 3), 0.25),
        "negative_diagonal": (-chain(11), 0.25),
        "mixed_diagonal": (sp.csr_matrix(mixed), 0.25),
        "all_equal_theta1": (torus(6), 1.0),                   # every coupling equals the maximum: the >= of the threshold
        "uneven_theta1": (uneven, 1.0),
        "theta0": (jit8, 0.0),
        "theta1": (jit8, 1.0),
        "diagonal": (sp.diags([np.arange(1.0, 6.0)], [0], format="csr"), 0.25),     # all FINE0, no coarse level
        "two_blocks": (sp.block_diag([chain(6), P.poisson_2d_structured(4)[0]], format="csr"), 0.25),
        "torus12": (torus(12), 0.25),                          # all column counts tie
    }
    return {k: (R.canonical(A), th) for k, (A, th) in cases.items()}


def overflow_row():
    """(A, state, row): a matrix whose row 2 is fine under `state` with d_2 = a_22 + (the couplings of its sign) = inf.
    (d_i = 0 cannot be reached with finite entries: the couplings that are lumped carry the diagonal's sign, so
    |d_i| >= |a_ii| > 0; a d_i that is not finite is the refusal that can.)  The split is handed to the interpolation
    stage as it is, so the case does not depend on the hash."""
    big = 1.0e308
    A = sp.lil_matrix(chain(5))
    A[2, 0], A[2, 4] = big, big
    A[2, 2] = big
    state = np.array([R.FINE, R.COARSE, R.FINE, R.COARSE, R.FINE], dtype=np.int32)
    return R.canonical(sp.csr_matrix(A)), state, 2


AMG_KW = dict(max_coarse=100)                                   # three or more levels at 33^2
CYCLE = dict(smoother="Jacobi", steps=2, omega=0.8)              # V(2,2) damped Jacobi
TARGET, CAP = 1e-8, 30


@functools.lru_cache(maxsize=None)
def twin_hierarchy(name, **kw):
    """(transfers, operators, info) of the twin on problems()[name]."""
    return R.classical_transfers(problems()[name][0], **dict(AMG_KW, **kw))


def oracle_history(A, b, Ps, cap=CAP, smoother="Jacobi", steps=2, omega=0.8, target=TARGET):
    """[||b - A x_k||] of the oracle's cycles on the transfers Ps from x_0 = 0, up to the first k with a norm at or below
    target * ||b||, at most cap cycles.  The norms are the oracle's own (kernels.residual)."""
    A = K.as_csr(A)
    h = V.HoistedVCycle(A, Ps)
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float64).ravel())
    x = np.zeros(A.shape[0])
    norm = lambda: float(np.sqrt(K.residual(A, x, b)[1]))
    hist = [norm()]
    while hist[-1] > target * hist[0] and len(hist) <= cap:
        x = h.cycle(x, b, smoother, steps, omega)
        hist.append(norm())
    return hist


def cycles_needed(hist, target=TARGET):
    """The number of cycles after which the history is at or below target * ||b||, or None."""
    return len(hist) - 1 if hist[-1] <= target * hist[0] else None
