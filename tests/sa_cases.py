"""TEST-ONLY: the matrices the smoothed-aggregation tests run on (tests/test_sa_cpu.py, tests/test_sa_gpu.py) and the twin's
whole hierarchies on the five 33^2 problems of amg_cases.  Nothing in learnmultigrid_amd imports this file."""
import functools

import numpy as np
import scipy.sparse as sp

import amg_cases as C
import sa_ref as R
from learnmultigrid_amd import problems as P

problems, chain, torus, oracle_history, cycles_needed = C.problems, C.chain, C.torus, C.oracle_history, C.cycles_needed

SA_KW = dict(max_coarse=100)                                    # as amg_cases.AMG_KW: 1089 -> 140 -> 9 on the grid problems
THETA = {"poisson": 0.0, "jittered": 0.0, "renumbered": 0.0, "variable": 0.0, "anisotropic": 0.25}
TARGET, CAP = C.TARGET, 60


def star(leaves):
    """Node 0 coupled to `leaves` leaves: one row of G with `leaves` entries, every leaf within one edge of the hub."""
    n = leaves + 1
    A = sp.lil_matrix((n, n))
    A.setdiag(np.concatenate([[float(leaves)], np.ones(leaves)]))
    A[0, 1:] = -1.0
    A[1:, 0] = -1.0
    return sp.csr_matrix(A)


def dirichlet_chain3():
    """[-1, 2, -1] on three nodes with identity end rows: the ends are isolated, the middle node keeps both couplings (its
    row of S has the two ends), has no neighbour in G and is a singleton aggregate."""
    return sp.csr_matrix(np.array([[1.0, 0.0, 0.0], [-1.0, 2.0, -1.0], [0.0, 0.0, 1.0]]))


def wavy(n):
    """A candidate that is not constant and nowhere zero."""
    return 1.0 + 0.5 * np.sin(0.7 * np.arange(n)) + np.arange(n) / (3.0 * n)


@functools.lru_cache(maxsize=None)
def case_matrices():
    """name -> (A, theta, B or None): the case matrices of amg_cases at their thetas, and the smallest shapes at which the
    aggregation kernels can go wrong."""
    jit8 = R.canonical(P.jittered_poisson_2d(8)[0])
    cases = {k: (A, th, None) for k, (A, th) in C.case_matrices().items()}
    cases.update({
        "chain5": (chain(5), 0.0, None),                           # the end nodes are two edges from the root: phase 2
        "dirichlet_chain3": (dirichlet_chain3(), 0.0, None),
        "star300": (star(300), 0.0, None),
        "jit8_theta0": (jit8, 0.0, None),
        "jit8_theta025": (jit8, 0.25, None),
        "jit8_theta1": (jit8, 1.0, None),
        "dirichlet_rows": (P.poisson_2d_structured(6)[0], 0.0, None),          # identity boundary rows: S is not symmetric
        "wavy_B": (jit8, 0.0, wavy(jit8.shape[0])),
        "wavy_B_chain257": (chain(257), 0.0, wavy(257)),
    })
    return {k: (R.canonical(A), th, B) for k, (A, th, B) in cases.items()}


def candidate(name):
    A, _, B = case_matrices()[name]
    return np.ones(A.shape[0]) if B is None else B


def zero_candidate():
    """(A, B, row): chain(9) with a candidate that is zero on the whole aggregate of node 4 and one elsewhere; `row` is
    the smallest member of that aggregate, the row both sides refuse with."""
    A = R.canonical(chain(9))
    agg = R.aggregate(R.symmetric_strength(A, 0.0))[0]
    B = np.where(agg == agg[4], 0.0, 1.0)
    return A, B, int(np.flatnonzero(agg == agg[4])[0])


@functools.lru_cache(maxsize=None)
def twin_hierarchy(name, theta=None, **kw):
    """(transfers, operators, info) of the twin on problems()[name], at THETA[name] unless theta is given."""
    th = THETA[name] if theta is None else theta
    return R.sa_transfers(problems()[name][0], theta=th, **dict(SA_KW, **kw))


def complexity(As):
    return sum(M.nnz for M in As) / As[0].nnz
