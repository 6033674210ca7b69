"""What the variant tests of the sweep kernels share (test_sell_variants_gpu.py, test_pcsr_variants_gpu.py,
test_fused_decomposition_gpu.py; no kernel reads this file): tune keys set for the length of a `with` block, output vectors
with a guarded tail, random matrices with prescribed row lengths, and the one checker that runs SpMV, residual and Jacobi
through ops.csr_* against oracle.kernels on the CSR matrix -- bit for bit."""
import contextlib
import functools

import numpy as np
import scipy.sparse as sp
import torch

from learnmultigrid_amd import _lib, ops
from oracle import kernels as K
from support import DEV, dev                         # noqa: F401  (the variant tests read them from here)
F64 = torch.float64
GUARD = 64                     # elements behind every output vector ...
SENTINEL = -2.5e300            # ... that must still hold this after every launch
ALPHA_BETA = ((1.0, 0.0), (1.0, 1.0), (-0.5, 2.0))
OMEGAS = (1.0, 0.8)


@contextlib.contextmanager
def tuned(**keys):
    """Tune keys set for the block and put back afterwards, whatever happens inside.  (Read through the library itself:
    ops.tune_get takes a negative value -- the default of sell_nt -- for a status.)"""
    L = _lib.lib()
    old = {k: int(L.lmg_tune_get(k.encode())) for k in keys}
    try:
        for k, v in keys.items():
            ops.tune_set(k, v)
        yield
    finally:
        for k, v in old.items():
            ops.tune_set(k, v)


class Guarded:
    """An output vector of n elements that is the head of an allocation of n + GUARD: the tail holds SENTINEL and must
    keep it.  fill: the initial contents (an array), None = NaN (an element the kernel does not write, or reads although
    it must not, then shows)."""

    def __init__(self, n, fill=None):
        self.n = n
        self.buf = torch.full((n + GUARD,), SENTINEL, dtype=F64, device=DEV)
        self.out = self.buf[:n]
        if fill is None:
            self.out.fill_(float("nan"))
        else:
            self.out.copy_(dev(fill))
        assert self.out.is_contiguous() and self.out.data_ptr() == self.buf.data_ptr()

    def result(self, tag):
        h = self.buf.cpu().numpy()
        assert (h[self.n:] == SENTINEL).all(), (tag, "wrote behind the vector", np.flatnonzero(h[self.n:] != SENTINEL)[:8])
        return h[:self.n]


def rows_matrix(n, m, lens, diag, seed, values=None):
    """Sorted n x m CSR with lens[i] entries in row i at distinct random columns of [0, m); diag[i]: column i is one of
    them (else it is none of them).  values: None = standard normal, or an array the values are drawn from."""
    rng = np.random.default_rng(seed)
    R, C = [], []
    for i in range(n):
        L = int(lens[i])
        if L == 0:
            continue
        others = np.delete(np.arange(m), i) if i < m else np.arange(m)
        if diag[i]:
            cols = np.concatenate([[i], rng.choice(others, L - 1, replace=False)])
        else:
            cols = rng.choice(others, L, replace=False)
        R.append(np.full(L, i))
        C.append(cols)
    R, C = np.concatenate(R), np.concatenate(C)
    V = rng.standard_normal(R.size) if values is None else rng.choice(np.asarray(values, dtype=np.float64), R.size)
    A = K.as_csr(sp.csr_matrix((V, (R, C)), shape=(n, m)))
    assert np.array_equal(np.diff(A.indptr), lens) and A.nnz == R.size
    return A


class Problem:
    """A matrix, its vectors on host and device, and the oracle's result of every sweep -- computed once."""

    def __init__(self, A, seed):
        self.A = A
        n, m = A.shape
        rng = np.random.default_rng(seed)
        self.x, self.b, self.y0 = rng.standard_normal(m), rng.standard_normal(n), rng.standard_normal(n)
        self.spmv = {ab: K.spmv(A, self.x, self.y0, *ab) for ab in ALPHA_BETA}
        if n == m:
            self.r, self.norm2 = K.residual(A, self.x, self.b)
            self.jacobi = {w: K.jacobi(A, self.x, self.b, w) for w in OMEGAS}


def first_diff(got, want):
    return np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:8]


def check_sweeps(tag, dA, pr, spmv_only=False):
    """The three SpMV forms, the residual with and without r, and two Jacobi sweeps on whatever twin dA carries: every
    vector equal to the oracle's, the squared norm to 1e-13 (another summation tree) and equal between the two residual
    runs.  Outputs start as NaN wherever the kernel must not read them (beta = 0, r, the Jacobi result)."""
    n, m = dA.shape
    dx, db = dev(pr.x), dev(pr.b)
    for (alpha, beta), want in pr.spmv.items():
        y = Guarded(n, None if beta == 0.0 else pr.y0)
        ops.csr_spmv(dA, dx, y.out, alpha, beta)
        got = y.result((tag, "spmv", alpha, beta))
        assert not np.isnan(got).any(), (tag, "spmv", alpha, beta, "NaN at", np.flatnonzero(np.isnan(got))[:8])
        assert np.array_equal(got, want), (tag, "spmv", alpha, beta, first_diff(got, want))
    if spmv_only or n != m:
        return
    r = Guarded(n)
    part = torch.empty(ops.partials_count(n), dtype=F64, device=DEV)
    n2, n2b = torch.zeros(1, dtype=F64, device=DEV), torch.zeros(1, dtype=F64, device=DEV)
    ops.csr_residual_norm2(dA, dx, db, r.out, part, n2)
    got = r.result((tag, "residual"))
    assert np.array_equal(got, pr.r), (tag, "residual", first_diff(got, pr.r))
    assert abs(n2.item() - pr.norm2) <= 1e-13 * pr.norm2, (tag, "norm2", n2.item(), pr.norm2)
    ops.csr_residual_norm2(dA, dx, db, None, part, n2b)
    assert n2b.item() == n2.item(), (tag, "norm2 without r", n2b.item(), n2.item())
    for omega, want in pr.jacobi.items():
        out = Guarded(n)
        ops.csr_jacobi(dA, dx, db, omega, out.out)
        got = out.result((tag, "jacobi", omega))
        assert np.array_equal(got, want), (tag, "jacobi", omega, first_diff(got, want))


# ---- the sliced-ELL cases: the fp64 and the fp32 variant tests run the same ones -------------------------------------------
SELL_JUS = (0, 5, 7, 8, 10)
SELL_NTS = (0, 1)
SELL_UNIFORM = (13, 35, 40, 41)
SELL_CASES = ["uniform_%d" % L for L in SELL_UNIFORM] + ["short_9", "ragged_slices"]


def sell_ragged_rows():
    """(row lengths, diagonal present) of the ragged case, slice by slice."""
    n = 321
    i = np.arange(64)
    lens = np.concatenate([
        np.full(64, 20),                              # slice 0: uniform
        (i * 7) % 31,                                 # slice 1: every length 0 .. 30, in no order
        np.zeros(64, dtype=np.int64),                 # slice 2: nothing at all
        (i % 3 == 0).astype(np.int64),                # slice 3: the longest row has one entry, two of three have none
        np.where(i % 5 == 2, 0, 30),                  # slice 4: empty rows between long ones
        [17]])                                        # slice 5: one row
    rows = np.arange(n)
    diag = (lens > 0) & ~((rows // 64 == 1) & (rows % 2 == 1)) & ~((rows // 64 == 3) & (rows % 2 == 1))
    assert lens.size == n and set(lens[64:128]) == set(range(31))
    return lens, diag


@functools.lru_cache(maxsize=None)
def sell_problem(name):
    if name.startswith("uniform_"):
        L, n = int(name.split("_")[1]), 200
        lens, diag = np.full(n, L), np.ones(n, dtype=bool)
    elif name == "short_9":
        n = 130
        lens, diag = np.full(n, 9), np.ones(n, dtype=bool)
    else:
        lens, diag = sell_ragged_rows()
        n = lens.size
    A = rows_matrix(n, n, lens, diag, seed=100 + n + int(lens.max()))
    return Problem(A, seed=n)
