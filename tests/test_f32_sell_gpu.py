"""Every compiled sliced-ELL sweep on an fp32 value stream (csrc/sell.hip, lmg_sell_sweep_f32), bit for bit (-m gpu).

The contract: a twin built with values="f32" IS the matrix A32 = double(float(A)), value by value; a value is widened when
it is loaded and the rest is the fp64 sweep.  So the twin is built from the UNROUNDED matrix, the oracle runs on the matrix
rounded to fp32 and back, and every vector must be equal -- no tolerance.  The cases, the guarded outputs and the checker
are those of test_sell_variants_gpu.py (sweep_variants.check_sweeps); sell_ju / sell_nt force every instantiation."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sweep_variants as SV                                          # noqa: E402
from learnmultigrid_amd import ops                                   # noqa: E402
from oracle import kernels as K                                      # noqa: E402  (checker only)

DEV = SV.DEV
CASES, JUS, NTS, problem = SV.SELL_CASES, SV.SELL_JUS, SV.SELL_NTS, SV.sell_problem


def rounded(A):
    B = A.copy()
    B.data = B.data.astype(np.float32).astype(np.float64)
    return B


@functools.lru_cache(maxsize=None)
def problem32(name):
    """The unrounded matrix of the fp64 case and the oracle's results on A32 -- with the vectors of the fp64 case."""
    pr = problem(name)
    pr32 = SV.Problem(rounded(pr.A), seed=pr.A.shape[0])
    assert np.array_equal(pr32.x, pr.x) and np.array_equal(pr32.b, pr.b)
    return pr.A, pr32, pr


@functools.lru_cache(maxsize=None)
def packable():
    """256 rows of 40 entries: four full slices, so that pack() itself picks the sliced-ELL twin (long rows whose values go
    raw; the 200-row cases end in a slice of 8 rows, whose padding pack() refuses)."""
    n = 256
    return SV.rows_matrix(n, n, np.full(n, 40), np.ones(n, dtype=bool), seed=256)


def sell32_operator(A, colmode):
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    S = ops.SellCSR.from_csr(dA, colmode=colmode, max_padding=float("inf"), values="f32")
    assert S is not None and S.values == "f32" and S.val.dtype == torch.float32
    dA.sell = S
    assert dA.patterns is None and dA.stencil is None and dA.packed is None and ops._PACKED_ENABLED
    return dA, S


@pytest.mark.parametrize("colmode", [0, 1], ids=["col16", "col32"])
@pytest.mark.parametrize("name", CASES)
def test_every_sell_kernel_on_fp32_values_bit_exact(name, colmode):
    A, pr32, pr64 = problem32(name)
    dA, S = sell32_operator(A, colmode)
    nsl = (A.shape[0] + 63) // 64
    assert S.bytes() == S.padded * ((2, 4)[colmode] + 4) + 16 * nsl + 4 * A.shape[0]
    S64 = ops.SellCSR.from_csr(ops.DeviceCSR.from_scipy(A, DEV), colmode=colmode, max_padding=float("inf"))
    assert S64.values == "f64" and S64.bytes() - S.bytes() == 4 * S.padded
    # the stream holds the rounded entries (padding: zeros)
    val = S.val.cpu().numpy()
    assert np.array_equal(np.sort(val[val != 0]), np.sort(A.data.astype(np.float32)))
    for ju in JUS:
        for nt in NTS:
            with SV.tuned(sell_ju=ju, sell_nt=nt):
                SV.check_sweeps((name, colmode, "f32", "sell_ju", ju, "sell_nt", nt), dA, pr32)
    # random values: A32 is another matrix than A, and a kernel that read an fp64 stream would not give A32's bits
    assert not np.array_equal(pr32.jacobi[0.8], pr64.jacobi[0.8])
    assert not np.array_equal(pr32.spmv[(1.0, 0.0)], pr64.spmv[(1.0, 0.0)])


@pytest.mark.parametrize("colmode", [0, 1], ids=["col16", "col32"])
def test_new_values_keep_the_twin_and_its_width(colmode):
    A, pr32, _ = problem32("ragged_slices")
    dA, S = sell32_operator(A, colmode)
    B = A.copy()
    B.data = np.random.default_rng(7).standard_normal(B.nnz)
    dA.vals.copy_(SV.dev(B.data))
    dA.repack_values()
    assert dA.sell is S and S.values == "f32" and S.val.dtype == torch.float32
    want = K.jacobi(rounded(B), pr32.x, pr32.b, 0.8)
    for ju in (7, 10):
        with SV.tuned(sell_ju=ju):
            out = SV.Guarded(B.shape[0])
            ops.csr_jacobi(dA, SV.dev(pr32.x), SV.dev(pr32.b), 0.8, out.out)
            got = out.result(("update_values", ju))
            assert np.array_equal(got, want), (ju, SV.first_diff(got, want))
    # values that leave the range: update_values refuses, repack_values builds that twin again in fp64
    B.data[5] = 1e-50
    dA.vals.copy_(SV.dev(B.data))
    assert S.update_values(dA) is False
    dA.repack_values()
    assert dA.sell is not S and dA.sell.values == "f64"
    out = SV.Guarded(B.shape[0])
    ops.csr_jacobi(dA, SV.dev(pr32.x), SV.dev(pr32.b), 0.8, out.out)
    assert np.array_equal(out.result("fp64 again"), K.jacobi(B, pr32.x, pr32.b, 0.8))


@pytest.mark.parametrize("value", [1e-50, 1e-39, 1e39, float("inf"), float("nan")],
                         ids=["to_zero", "to_subnormal", "to_inf", "inf", "nan"])
def test_a_value_that_rounding_would_change_refuses_the_twin(value):
    A = packable().copy()
    A.data[1234] = value
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    assert ops.SellCSR.from_csr(dA, values="f32") is None
    assert ops.SellCSR.from_csr(dA, colmode=1, values="f32") is None
    dA.pack(values="f32")
    assert dA.values == "f32" and dA.twin_values == "f64"
    assert dA.sell is not None and dA.sell.values == "f64" and dA.sell.val.dtype == torch.float64
    if np.isfinite(value):
        SV.check_sweeps(("fp64 fallback", value), dA, SV.Problem(A, seed=256))


def test_pack_picks_an_fp32_sell_twin_and_explicit_zeros_are_fine():
    A = packable().copy()
    A.data[77] = 0.0
    A.data[78] = -0.0
    assert A.nnz == 256 * 40                                          # stored, not eliminated
    dA = ops.DeviceCSR.from_scipy(A, DEV, canonical=False)
    dA.pack(values="f32")
    assert dA.twin_values == "f32" and dA.sell is not None and dA.sell.values == "f32" and dA.packed is None
    SV.check_sweeps("explicit zeros", dA, SV.Problem(rounded(A), seed=256))
    with pytest.raises(ValueError, match="f16"):
        dA.pack(values="f16")
    with pytest.raises(ValueError, match="f16"):
        ops.SellCSR.from_csr(dA, values="f16")
