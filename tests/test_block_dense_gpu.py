"""ops.dense_gemv_block (csrc/dense.hip: dense_gemv_block_kernel), the coarsest-level solve on a block of right-hand
sides (-m gpu): Y = M X within the rounding bound of a row sum, columns independent of each other, deterministic, nothing
written behind the block, and -- where lmg_dense_gemv runs its one-wave-per-row kernel -- column j bit for bit what
ops.dense_gemv gives on column j."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from learnmultigrid_amd import ops                                   # noqa: E402
from support import DEV, dev                                         # noqa: E402
from sweep_variants import GUARD, SENTINEL                           # noqa: E402

F64 = torch.float64
EPS = float(np.finfo(np.float64).eps)
# odd m (elements per lane), even m past one trip of the wave (128 elements), the smallest even row, m = 2 (mod 4)
SHAPES = [(81, 81), (130, 258), (1, 2), (289, 290)]


def one_wave_per_row(n, m):
    """The size rule of lmg_dense_gemv (csrc/dense.hip): `n <= 8192 && m >= 1024` goes to the workgroup-per-row kernel,
    which adds four partial sums per row and rounds differently; every other shape runs dense_gemv_kernel."""
    return not (n <= 8192 and m >= 1024)


def guarded(n, k):
    buf = torch.full((n * k + GUARD,), SENTINEL, dtype=F64, device=DEV)
    out = buf[:n * k].view(n, k)
    out.fill_(float("nan"))
    return buf, out


def result(buf, n, k):
    h = buf.cpu().numpy()
    assert (h[n * k:] == SENTINEL).all(), "wrote behind the block"
    return h[:n * k].reshape(n, k)


@pytest.mark.parametrize("k", ops.BLOCK_WIDTHS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_dense_gemv_block(n, m, k):
    rng = np.random.default_rng(1000 * n + m)
    M, X = rng.standard_normal((n, m)), rng.standard_normal((m, k))
    dM, dX = dev(M), dev(X)
    buf, Y = guarded(n, k)
    ops.dense_gemv_block(dM, dX, Y)
    got = result(buf, n, k)
    # a sum of m rounded products is within gamma_m (|M| |x|) of the exact one in any order, gamma_m = m u / (1 - m u) with
    # u = EPS / 2; that holds for the kernel and for NumPy's product, so the two differ by at most 2 gamma_m < 2 m EPS
    bound = 2 * m * EPS * (np.abs(M) @ np.abs(X))
    assert not np.isnan(got).any()
    assert (np.abs(got - M @ X) <= bound).all(), np.abs(got - M @ X).max()
    buf2, Y2 = guarded(n, k)
    ops.dense_gemv_block(dM, dX, Y2)
    assert np.array_equal(result(buf2, n, k), got)                           # deterministic
    assert one_wave_per_row(n, m)
    y = torch.full((n,), np.nan, dtype=F64, device=DEV)
    for j in range(k):                                                         # the single-vector kernel on column j
        ops.dense_gemv(dM, dX[:, j].contiguous(), y)
        assert np.array_equal(y.cpu().numpy(), got[:, j]), (j, np.flatnonzero(y.cpu().numpy() != got[:, j])[:8])
    for j in (0, k - 1):                                                       # the other columns do not reach column j
        X3 = 1e3 * rng.standard_normal((m, k))
        X3[:, j] = X[:, j]
        buf3, Y3 = guarded(n, k)
        ops.dense_gemv_block(dM, dev(X3), Y3)
        assert np.array_equal(result(buf3, n, k)[:, j], got[:, j]), j


def test_dense_gemv_block_checks_its_blocks():
    M = torch.zeros((6, 4), dtype=F64, device=DEV)
    X, Y = torch.zeros((4, 4), dtype=F64, device=DEV), torch.zeros((6, 4), dtype=F64, device=DEV)
    with pytest.raises(ValueError):
        ops.dense_gemv_block(M, X, torch.zeros((6, 2), dtype=F64, device=DEV))
    with pytest.raises(ValueError):
        ops.dense_gemv_block(M, X[:3], Y)
    with pytest.raises(ValueError):
        ops.dense_gemv_block(M, torch.zeros((4, 3), dtype=F64, device=DEV), torch.zeros((6, 3), dtype=F64, device=DEV))
    with pytest.raises(TypeError):
        ops.dense_gemv_block(M, X.to(torch.float32), Y)
