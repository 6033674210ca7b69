"""The three kernels of conjugate gradients on blocks of right-hand sides (-m gpu), bit for bit against the single-vector
kernels they stand for: block_dot against dot, block_cg_step and block_cg_direction against axpby with coefficients divided
on the host, on columns copied out of the blocks.  n = 1, 255 (less than a workgroup), 1089 (several workgroups, odd) and
262144 + 257, the smallest n at which a lane of the fixed 1024 x 256 geometry makes a second trip."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from learnmultigrid_amd import ops                                   # noqa: E402
from support import DEV, dev                                         # noqa: E402

F64 = torch.float64
WIDTHS = (2, 4, 8)
SIZES = (1, 255, 1089, 262144 + 257)
CASES = [(k, n) for k in WIDTHS for n in SIZES]


def blocks(n, k, count, seed):
    rng = np.random.default_rng(seed)
    return [dev(rng.standard_normal((n, k))) for _ in range(count)]


def scalars(*rows):
    """One device array per row of host values."""
    return [dev(np.array(r, dtype=np.float64)) for r in rows]


def column(T, j):
    """Column j in an allocation of its own (a one-row view counts as contiguous where it stands, 8 bytes off alignment)."""
    return T[:, j].clone(memory_format=torch.contiguous_format)


def single_dot(x, y):
    part = torch.empty(ops.partials_count(x.numel()), dtype=F64, device=DEV)
    out = torch.zeros(1, dtype=F64, device=DEV)
    ops.dot(x, y, part, out)
    return out.item()


def run_block_dot(X, Y):
    n, k = X.shape
    part = torch.full((ops.block_dot_partials_count(n, k),), np.nan, dtype=F64, device=DEV)
    out = torch.full((k,), np.nan, dtype=F64, device=DEV)
    ops.block_dot(X, Y, part, out)
    return out.cpu().numpy()


def single_axpby(alpha, x, beta, y):
    y = y.clone()
    ops.axpby(alpha, x, beta, y)
    return y.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("k,n", CASES)
def test_block_dot_has_the_bits_of_dot_on_every_column(k, n):
    X, Y = blocks(n, k, 2, seed=n + k)
    got = run_block_dot(X, Y)
    want = np.array([single_dot(column(X, j), column(Y, j)) for j in range(k)])
    assert np.array_equal(got, want)
    assert np.array_equal(run_block_dot(X, X), np.array([single_dot(column(X, j), column(X, j)) for j in range(k)]))
    assert ops.block_dot_partials_count(n, k) == 1024 * k


@pytest.mark.parametrize("k,n", CASES)
def test_block_cg_step_has_the_bits_of_two_axpby_and_a_dot(k, n):
    Pb, AP, X, R = blocks(n, k, 4, seed=3 * n + k)
    off = 1                                                           # the frozen column: NaN wherever it must not be read
    Pb[:, off] = np.nan
    AP[:, off] = np.nan
    rng = np.random.default_rng(k)
    h_rz, h_pAp = rng.uniform(0.5, 2.0, k), rng.uniform(0.5, 2.0, k)
    h_mask = np.ones(k)
    h_mask[off] = 0.0
    rz, pAp, tol2, mask = scalars(h_rz, h_pAp, np.zeros(k), h_mask)
    want_x, want_r = X.cpu().numpy().copy(), R.cpu().numpy().copy()
    for j in range(k):
        if j != off:
            alpha = float(h_rz[j]) / float(h_pAp[j])
            want_x[:, j] = single_axpby(alpha, column(Pb, j), 1.0, column(X, j))
            want_r[:, j] = single_axpby(-alpha, column(AP, j), 1.0, column(R, j))
    part = torch.empty(ops.block_dot_partials_count(n, k), dtype=F64, device=DEV)
    rr = torch.full((k,), np.nan, dtype=F64, device=DEV)
    ops.block_cg_step(rz, pAp, tol2, mask, Pb, AP, X, R, part, rr)
    assert np.array_equal(bits(X.cpu().numpy()), bits(want_x))        # the frozen column kept its bits
    assert np.array_equal(bits(R.cpu().numpy()), bits(want_r))
    assert np.array_equal(rr.cpu().numpy(), run_block_dot(R, R))
    assert np.array_equal(mask.cpu().numpy(), h_mask)                 # rr > 0 = tol2: what was on stays on, off stays off


@pytest.mark.parametrize("k,n", CASES)
def test_block_cg_direction_has_the_bits_of_axpby(k, n):
    Z, Pb = blocks(n, k, 2, seed=5 * n + k)
    # pairs of columns share a 16-byte store: (off, on) at k = 2; (off, on), (off, off) and whole pairs at k = 4 and 8
    off = (0,) if k == 2 else (0, 2, 3)
    for j in off:
        Z[:, j] = np.nan
    rng = np.random.default_rng(k + 1)
    h_new, h_old = rng.uniform(0.5, 2.0, k), rng.uniform(0.5, 2.0, k)
    h_new[1] = 0.0                                                    # beta = 0: p = z, like axpby
    h_mask = np.ones(k)
    h_mask[list(off)] = 0.0
    rz_new, rz_old, mask = scalars(h_new, h_old, h_mask)
    want = Pb.cpu().numpy().copy()
    for j in range(k):
        if j not in off:
            want[:, j] = single_axpby(1.0, column(Z, j), float(h_new[j]) / float(h_old[j]), column(Pb, j))
    ops.block_cg_direction(rz_new, rz_old, mask, Z, Pb)
    assert np.array_equal(bits(Pb.cpu().numpy()), bits(want))
    assert np.array_equal(mask.cpu().numpy(), h_mask)


@pytest.mark.parametrize("k", WIDTHS)
def test_the_mask_update_at_the_threshold_and_a_zero_pAp(k):
    """pAp = 0 everywhere: alpha = 0 instead of rz / 0, x and r keep their values, rr is |r|^2 as it stands.  Thresholds at
    rr, one ulp below and one above: only a column that is on and strictly above its threshold stays on."""
    n = 1089
    Pb, AP, X, R = blocks(n, k, 4, seed=77 + k)
    x0, r0 = X.cpu().numpy().copy(), R.cpu().numpy().copy()
    rr0 = run_block_dot(R, R)
    h_tol2 = np.array([[np.nextafter(rr0[j], -np.inf), rr0[j], np.nextafter(rr0[j], np.inf)][j % 3] for j in range(k)])
    h_mask = np.ones(k)
    if k > 2:
        h_mask[3] = 0.0                                               # above its threshold, but off: stays off
    rz, pAp, tol2, mask = scalars(np.full(k, 1.5), np.zeros(k), h_tol2, h_mask)
    part = torch.empty(ops.block_dot_partials_count(n, k), dtype=F64, device=DEV)
    rr = torch.full((k,), np.nan, dtype=F64, device=DEV)
    ops.block_cg_step(rz, pAp, tol2, mask, Pb, AP, X, R, part, rr)
    assert np.array_equal(X.cpu().numpy(), x0) and np.array_equal(R.cpu().numpy(), r0)
    assert np.array_equal(rr.cpu().numpy(), rr0)
    want = [1.0 if (j % 3 == 0 and h_mask[j] != 0.0) else 0.0 for j in range(k)]
    assert want == {2: [1.0, 0.0], 4: [1.0, 0.0, 0.0, 0.0], 8: [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]}[k]
    assert mask.cpu().tolist() == want


def test_wrappers_refuse_what_the_kernels_cannot_take():
    X, Y = blocks(64, 4, 2, seed=1)
    part = torch.empty(1024 * 4, dtype=F64, device=DEV)
    out = torch.zeros(4, dtype=F64, device=DEV)
    with pytest.raises(ValueError):
        ops.block_dot(X, Y[:, :2].contiguous(), part, out)
    with pytest.raises(ValueError):
        ops.block_dot(X, Y, part[:100], out)
    with pytest.raises(ValueError):
        ops.block_dot(X, Y, part, out[:2])
    with pytest.raises(ops.LmgError):
        ops.block_cg_direction(out, out, out, X, Y)                   # rz_new is rz_old
    with pytest.raises(ops.LmgError):
        ops.block_cg_direction(out, out.clone(), out, X, X)
