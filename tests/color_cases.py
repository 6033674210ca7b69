"""TEST-ONLY: the matrices the tests of the "multicolor_device" Gauss-Seidel ordering run on (tests/test_color_cpu.py,
tests/test_color_gpu.py) -- the smallest at which the kernels can go wrong -- and the twin's colouring of each, computed once.
Nothing in learnmultigrid_amd imports this file."""
import functools

import numpy as np
import scipy.sparse as sp

import amg_cases as C
import color_ref as K
from learnmultigrid_amd import problems as P


def star(leaves):
    """Node 0 coupled to `leaves` leaves: degree >= 64 with two colours."""
    n = leaves + 1
    rows = np.concatenate([np.zeros(leaves, dtype=int), np.arange(1, n), np.arange(n)])
    cols = np.concatenate([np.arange(1, n), np.zeros(leaves, dtype=int), np.arange(n)])
    vals = np.concatenate([-np.ones(2 * leaves), float(leaves) * np.ones(n)])
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n))


def complete(n):
    return sp.csr_matrix(np.full((n, n), -1.0) + (n + 1.0) * np.eye(n))


def dirichlet_rows():
    """chain(12) with rows 0, 5 and 11 replaced by identity rows whose columns stay: an unsymmetric pattern."""
    A = sp.lil_matrix(C.chain(12))
    for i in (0, 5, 11):
        A[i, :] = 0.0
        A[i, i] = 1.0
    return sp.csr_matrix(A)


@functools.lru_cache(maxsize=None)
def case_matrices():
    pr = C.problems()
    cases = {
        "poisson8": P.poisson_2d_structured(8)[0],
        "jittered32": pr["jittered"][0],
        "renumbered32": pr["renumbered"][0],
        "level1": C.twin_hierarchy("jittered")[1][1],              # rows of about 23 entries
        "chain257": C.chain(257),                                  # one lane in the second workgroup
        "torus12": C.torus(12),
        "n1": sp.csr_matrix(np.array([[2.0]])),
        "n0": sp.csr_matrix((0, 0)),
        "diagonal": sp.diags([np.arange(1.0, 6.0)], [0], format="csr"),
        "dirichlet_rows": dirichlet_rows(),
        "star70": star(70),
        "complete64": complete(64),
    }
    return {k: sp.csr_matrix(A, dtype=np.float64) for k, A in cases.items()}


@functools.lru_cache(maxsize=None)
def coloring(name):
    return K.color(case_matrices()[name])


CASES = ("poisson8", "jittered32", "renumbered32", "level1", "chain257", "torus12", "n1", "n0", "diagonal", "dirichlet_rows",
         "star70", "complete64")
