"""The fused passes of csrc/dia_tile.hip on fp32 slot arrays (lmg_dia_smooth_f32, lmg_dia_cheby_f32), bit for bit (-m gpu).

The twin is built with values="f32" from the unrounded matrix and must be A32 = double(float(A)), value by value: the Jacobi
passes against the CPU oracle's separate sweeps and residual on A32, a Chebyshev step against the two-launch path on an
fp64 twin of A32.  No tolerance anywhere.  Sizes: the smallest above DiaTwin.MIN_ROWS (65 x 65), one matrix per slot set
of 5, 7 and 9 slots; several tiles in both directions for either tile height."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from learnmultigrid_amd import ops, problems as P                           # noqa: E402
from learnmultigrid_amd.hierarchy import chebyshev_coefficients             # noqa: E402
from oracle import kernels as K                                             # noqa: E402  (checker only)
from support import DEV, dev, nan_vec                                       # noqa: E402

NAMES = ("jittered7_65", "varcoeff5_65", "perturbed9_65")
OMEGAS = (0.8, 1.0)


def rounded(A):
    B = A.copy()
    B.data = B.data.astype(np.float32).astype(np.float64)
    return B


@functools.lru_cache(maxsize=None)
def case(name):
    """(A, A32, x0, b, want): want[(omega, zero)] = [(x after S sweeps, its residual) for S = 1, 2, 3], the oracle on A32 --
    computed once for both tile heights."""
    if name == "jittered7_65":
        A = K.as_csr(P.jittered_poisson_2d(64)[0])
    elif name == "varcoeff5_65":
        A = K.as_csr(P.variable_coeff_poisson_2d_structured(64)[0])
    else:
        A0 = P.poisson_2d_structured(128)[0]
        Pm = P.tensor_interpolator_2d(129)
        G = sp.csr_matrix(Pm.T @ A0 @ Pm)
        G.sort_indices()
        G.data = G.data * (1.0 + 0.1 * np.random.default_rng(3).random(G.nnz))     # 9-point, every value distinct
        A = K.as_csr(G)
    n = A.shape[0]
    assert n == 65 * 65 and n >= ops.DiaTwin.MIN_ROWS
    A32 = rounded(A)
    assert not np.array_equal(A32.data, A.data)
    rng = np.random.default_rng(77)
    x0, b = rng.standard_normal(n), rng.standard_normal(n)
    want = {}
    for omega in OMEGAS:
        for zero in (False, True):
            x, steps = (np.zeros(n) if zero else x0.copy()), []
            for _ in range(3):
                x = K.jacobi(A32, x, b, omega)
                steps.append((x, K.residual(A32, x, b)[0]))
            want[(omega, zero)] = steps
    return A, A32, x0, b, want


def packed32(A):
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dA.pack(values="f32")
    D = dA.dia
    assert dA.twin_values == "f32" and dA.stencil is None and D is not None and D.values == "f32"
    assert D.dia.dtype == torch.float32 and D.bytes() == 4 * D.nslots * A.shape[0]
    return dA, D


@pytest.mark.parametrize("name,nslots", zip(NAMES, (7, 5, 9)))
@pytest.mark.parametrize("rows", [32, 64])
def test_fp32_dia_passes_equal_the_oracle_on_the_rounded_matrix(name, nslots, rows):
    A, A32, x0, b, want = case(name)
    n = A.shape[0]
    dA, D = packed32(A)
    assert D.nslots == nslots and D.W == 65 and ops._fused_kind(dA) == "dia"
    # the twin is A32: slot arrays against the rounded CSR entries
    coo = A.tocoo()
    slots = [s for s in range(9) if (D.umask >> s) & 1]
    dia = D.dia.cpu().numpy().reshape(len(slots), n)
    off = coo.col.astype(np.int64) - coo.row
    for q, s in enumerate(slots):
        w = np.zeros(n, dtype=np.float32)
        m = off == (s // 3 - 1) * D.W + (s % 3 - 1)
        w[coo.row[m]] = coo.data[m].astype(np.float32)
        assert np.array_equal(dia[q], w), (name, s)
    # the fp64 twin of A gives other bits: a kernel that read fp64 slot arrays could not pass below
    assert not np.array_equal(K.jacobi(K.as_csr(A), x0, b, 0.8), want[(0.8, False)][0][0])
    try:
        ops.tune_set("dia_rows", rows)
        for omega in OMEGAS:
            for zero in (False, True):
                for S in (1, 2, 3):
                    wx, wr = want[(omega, zero)][S - 1]
                    for resid in (False, True):
                        out, r = nan_vec(n), (nan_vec(n) if resid else None)
                        ops.stencil_smooth(dA, None if zero else dev(x0), dev(b), omega, S, out, r)
                        got = out.cpu().numpy()
                        assert not np.isnan(got).any(), (name, S, zero, resid)
                        assert np.array_equal(got, wx), (name, omega, S, zero, resid, np.flatnonzero(got != wx)[:8])
                        if resid:
                            assert np.array_equal(r.cpu().numpy(), wr), (name, omega, S, zero)
    finally:
        ops.tune_set("dia_rows", 0)


def two_launch(dA, x0, b, coef):
    """A Chebyshev step as every format without a fused pass runs it: residual launch + lmg_cheby_update per sweep."""
    n = dA.shape[0]
    x = torch.zeros(n, dtype=torch.float64, device=DEV) if x0 is None else dev(x0)
    dinv = ops.csr_inverse_diagonal(dA)
    d, r, db = nan_vec(n), nan_vec(n), dev(b)
    for k, (a, c) in enumerate(coef):
        ops.csr_residual_norm2(dA, x, db, r, None, None)
        ops.cheby_update(a, c, dinv, r, d, x, first=(k == 0))
    return x.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("rows", [32, 64])
def test_fp32_chebyshev_step_equals_the_two_launch_path_on_an_fp64_twin_of_the_rounded_matrix(name, rows):
    A, A32, x0, b, _want = case(name)
    n = A.shape[0]
    dA, _D = packed32(A)
    d64 = ops.DeviceCSR.from_scipy(A32, DEV)
    d64.pack()
    assert d64.twin_values == "f64" and d64.dia is not None and d64.dia.values == "f64"
    g = torch.empty(1, dtype=torch.float64, device=DEV)
    ops.csr_gershgorin(d64, g)
    lmax = float(g.item())
    try:
        ops.tune_set("dia_rows", rows)
        for S in (1, 2, 3):
            coef = chebyshev_coefficients(lmax, 4.0, S)
            for zero in (False, True):
                want = two_launch(d64, None if zero else x0, b, coef)
                wr, _ = K.residual(A32, want, b)
                for resid in (False, True):
                    out, r = nan_vec(n), (nan_vec(n) if resid else None)
                    ops.stencil_cheby(dA, None if zero else dev(x0), dev(b), coef, out, r)
                    got = out.cpu().numpy()
                    assert np.array_equal(got, want), (name, S, zero, resid, np.flatnonzero(got != want)[:8])
                    if resid:
                        assert np.array_equal(r.cpu().numpy(), wr), (name, S, zero)
                    # ... and the fused fp64 pass on the fp64 twin of A32
                    out64 = nan_vec(n)
                    ops.stencil_cheby(d64, None if zero else dev(x0), dev(b), coef, out64, None)
                    assert np.array_equal(out64.cpu().numpy(), want)
    finally:
        ops.tune_set("dia_rows", 0)


@pytest.mark.parametrize("value", [1e-50, 1e39, float("inf")], ids=["to_zero", "to_inf", "inf"])
def test_a_value_that_rounding_would_change_refuses_the_fp32_slot_arrays(value):
    A = case("varcoeff5_65")[0].copy()
    A.data[A.indptr[2000]] = value
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    assert ops.DiaTwin.from_csr(dA, values="f32") is None
    assert ops.DiaTwin.from_csr(dA) is not None
    dA.pack(values="f32")
    assert dA.values == "f32" and dA.twin_values == "f64" and dA.dia is not None and dA.dia.values == "f64"
    with pytest.raises(ValueError, match="f16"):
        ops.DiaTwin.from_csr(dA, values="f16")


def test_new_values_keep_the_width_and_out_of_range_values_bring_fp64_back():
    A, _A32, x0, b, _want = case("jittered7_65")
    n = A.shape[0]
    dA, D = packed32(A)
    B = A.copy()
    B.data = B.data * (1.0 + 0.25 * np.random.default_rng(5).random(B.nnz))
    dA.vals.copy_(dev(B.data))
    dA.repack_values()
    assert dA.dia is D and D.values == "f32" and D.dia.dtype == torch.float32 and dA.twin_values == "f32"
    out = nan_vec(n)
    ops.stencil_smooth(dA, dev(x0), dev(b), 0.8, 1, out, None)
    assert np.array_equal(out.cpu().numpy(), K.jacobi(rounded(B), x0, b, 0.8))
    y = nan_vec(n)
    ops.csr_spmv(dA, dev(x0), y)                                    # the packed twin next to it applies A32 too
    assert np.array_equal(y.cpu().numpy(), K.spmv(rounded(B), x0, np.zeros(n), 1.0, 0.0))
    B.data[100] = 1e-60
    dA.vals.copy_(dev(B.data))
    assert D.update_values(dA) is False
    dA.repack_values()
    assert dA.values == "f32" and dA.twin_values == "f64" and dA.dia.values == "f64"
    ops.stencil_smooth(dA, dev(x0), dev(b), 0.8, 1, out, None)
    assert np.array_equal(out.cpu().numpy(), K.jacobi(K.as_csr(B), x0, b, 0.8))
