"""The sliced-ELL sweeps on blocks of k right-hand sides (csrc/sell.hip: sell_sweep_block_kernel) against the CPU oracle
on the CSR matrix, column by column and bit for bit (-m gpu).

36 kernels are compiled -- 3 modes x 2 column widths x k in {2, 4, 8} x (cached, nontemporal) -- and every one runs here:
on the sliced-ELL cases of the single-vector variant tests (sweep_variants.SELL_CASES: 200-, 130- and 321-row matrices,
ragged slices, empty rows, rows without a diagonal) and on a rectangular pair (200 x 77 with rows of at most 9 entries,
77 x 200 with 25-entry rows: SpMV only).  Column j of every output must equal oracle.kernels on column j; norm2[j] must
equal the single-vector sweep's norm2 on the same twin and column bit for bit.  Blocks are the head of a longer
allocation whose tail must keep its sentinel, and start as NaN wherever a kernel must not read them."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sweep_variants as SV                                          # noqa: E402
from learnmultigrid_amd import ops                                   # noqa: E402
from oracle import kernels as K                                      # noqa: E402  (checker only)

DEV, F64 = SV.DEV, torch.float64
KMAX = 8


class GuardedBlock:
    """An (n, k) block that is the head of an allocation of n * k + GUARD doubles whose tail holds SENTINEL.
    fill: the initial contents (an (n, k) array), None = NaN."""

    def __init__(self, n, k, fill=None):
        self.n, self.k = n, k
        self.buf = torch.full((n * k + SV.GUARD,), SV.SENTINEL, dtype=F64, device=DEV)
        self.out = self.buf[:n * k].view(n, k)
        if fill is None:
            self.out.fill_(float("nan"))
        else:
            self.out.copy_(SV.dev(fill))
        assert self.out.is_contiguous() and self.out.data_ptr() == self.buf.data_ptr() and self.out.data_ptr() % 16 == 0

    def result(self, tag):
        h = self.buf.cpu().numpy()
        tail = h[self.n * self.k:]
        assert (tail == SV.SENTINEL).all(), (tag, "wrote behind the block", np.flatnonzero(tail != SV.SENTINEL)[:8])
        return h[:self.n * self.k].reshape(self.n, self.k)


class BlockProblem:
    """KMAX columns of x, b and y0 for a matrix and the oracle's result of every sweep on every column -- computed once;
    a block of width k uses the first k columns."""

    def __init__(self, A, seed, first=None):
        self.A = A
        n, m = A.shape
        rng = np.random.default_rng(seed)
        self.X, self.B, self.Y0 = rng.standard_normal((m, KMAX)), rng.standard_normal((n, KMAX)), rng.standard_normal((n, KMAX))
        if first is not None:                                     # column 0: the vectors of the single-vector problem
            self.X[:, 0], self.B[:, 0], self.Y0[:, 0] = first.x, first.b, first.y0
        cols = range(KMAX)
        self.spmv = {ab: np.column_stack([K.spmv(A, self.X[:, j], self.Y0[:, j], *ab) for j in cols]) for ab in SV.ALPHA_BETA}
        if n == m:
            res = [K.residual(A, self.X[:, j], self.B[:, j]) for j in cols]
            self.r, self.norm2 = np.column_stack([r for r, _ in res]), np.array([n2 for _, n2 in res])
            self.jacobi = {w: np.column_stack([K.jacobi(A, self.X[:, j], self.B[:, j], w) for j in cols]) for w in SV.OMEGAS}
        if first is not None:
            assert np.array_equal(self.spmv[SV.ALPHA_BETA[2]][:, 0], first.spmv[SV.ALPHA_BETA[2]])


@functools.lru_cache(maxsize=None)
def block_problem(name):
    if name == "rect_tall":
        A = SV.rows_matrix(200, 77, np.random.default_rng(3).integers(0, 10, 200), np.zeros(200, dtype=bool), seed=277)
        return BlockProblem(A, seed=277)
    if name == "rect_wide":
        A = SV.rows_matrix(77, 200, np.full(77, 25), np.zeros(77, dtype=bool), seed=772)
        return BlockProblem(A, seed=772)
    pr = SV.sell_problem(name)
    return BlockProblem(pr.A, seed=pr.A.shape[0] + 1000, first=pr)


def twin(A, colmode):
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    S = ops.SellCSR.from_csr(dA, colmode=colmode, max_padding=float("inf"))
    assert S is not None and S.colmode == colmode and S.values == "f64"
    dA.sell = S
    assert ops.block_twin(dA) is S                                # an fp64 twin the matrix has is the one the block sweeps read
    return dA, S


def same(tag, got, want):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(got, want), (tag, [(j, SV.first_diff(got[:, j], want[:, j])) for j in range(got.shape[1])
                                             if not np.array_equal(got[:, j], want[:, j])][:3])


def blk(a, k):
    return SV.dev(np.ascontiguousarray(a[:, :k]))


def check_block_spmv(tag, S, bp, k):
    n = S.shape[0]
    dX = blk(bp.X, k)
    for (alpha, beta), want in bp.spmv.items():
        Y = GuardedBlock(n, k, None if beta == 0.0 else bp.Y0[:, :k])
        ops.block_spmv(S, dX, Y.out, alpha, beta)
        same((tag, "spmv", alpha, beta), Y.result((tag, "spmv", alpha, beta)), want[:, :k])


def check_block_sweeps(tag, dA, S, bp, k):
    """Every column of the three SpMV forms, the residual with and without R, norm2 against the single-vector sweep and
    the oracle, and two Jacobi sweeps."""
    n = S.shape[0]
    check_block_spmv(tag, S, bp, k)
    dX, dB = blk(bp.X, k), blk(bp.B, k)
    part = torch.full((ops.block_partials_count(n, k) + SV.GUARD,), SV.SENTINEL, dtype=F64, device=DEV)
    n2 = torch.full((k + 2,), SV.SENTINEL, dtype=F64, device=DEV)
    n2b = torch.full((k + 2,), SV.SENTINEL, dtype=F64, device=DEV)
    R = GuardedBlock(n, k)
    ops.block_residual_norm2(S, dX, dB, R.out, part[:-SV.GUARD], n2[:k])
    same((tag, "residual"), R.result((tag, "residual")), bp.r[:, :k])
    got = n2.cpu().numpy()
    assert (got[k:] == SV.SENTINEL).all() and (part[-SV.GUARD:].cpu().numpy() == SV.SENTINEL).all(), (tag, "norm2 / partials overrun")
    assert (np.abs(got[:k] - bp.norm2[:k]) <= 1e-13 * bp.norm2[:k]).all(), (tag, "norm2", got[:k], bp.norm2[:k])
    ops.block_residual_norm2(S, dX, dB, None, part[:-SV.GUARD], n2b[:k])
    assert np.array_equal(n2b.cpu().numpy(), got), (tag, "norm2 without R")
    spart = torch.empty(ops.partials_count(n), dtype=F64, device=DEV)
    s2 = torch.zeros(1, dtype=F64, device=DEV)
    for j in range(k):                                            # the single-vector SELL sweep on column j: the same bits
        ops.csr_residual_norm2(dA, dX[:, j].contiguous(), dB[:, j].contiguous(), None, spart, s2)
        assert s2.item() == got[j], (tag, "norm2 of column", j, s2.item(), got[j])
    for omega, want in bp.jacobi.items():
        Out = GuardedBlock(n, k)
        ops.block_jacobi(S, dX, dB, omega, Out.out)
        same((tag, "jacobi", omega), Out.result((tag, "jacobi", omega)), want[:, :k])


def check_independence(tag, S, bp, k):
    """Column j of every output keeps its bits when the other columns' inputs are replaced."""
    n, m = S.shape
    rng = np.random.default_rng(99)
    for j in (0, k - 1):
        X, B, Y0 = (np.ascontiguousarray(a[:, :k]).copy() for a in (bp.X, bp.B, bp.Y0))
        for a in (X, B, Y0):
            keep = a[:, j].copy()
            a[:] = 1e3 * rng.standard_normal(a.shape)
            a[:, j] = keep
        dX, dB = SV.dev(X), SV.dev(B)
        Y = GuardedBlock(n, k, Y0)
        ops.block_spmv(S, dX, Y.out, -0.5, 2.0)
        assert np.array_equal(Y.result((tag, "spmv", j))[:, j], bp.spmv[(-0.5, 2.0)][:, j]), (tag, "spmv column", j)
        if n != m:
            continue
        R, Out = GuardedBlock(n, k), GuardedBlock(n, k)
        part = torch.empty(ops.block_partials_count(n, k), dtype=F64, device=DEV)
        n2, ref2 = torch.zeros(k, dtype=F64, device=DEV), torch.zeros(k, dtype=F64, device=DEV)
        ops.block_residual_norm2(S, dX, dB, R.out, part, n2)
        ops.block_residual_norm2(S, blk(bp.X, k), blk(bp.B, k), None, part, ref2)
        assert np.array_equal(R.result((tag, "residual", j))[:, j], bp.r[:, j]) and n2[j].item() == ref2[j].item(), (tag, "residual", j)
        ops.block_jacobi(S, dX, dB, 0.8, Out.out)
        assert np.array_equal(Out.result((tag, "jacobi", j))[:, j], bp.jacobi[0.8][:, j]), (tag, "jacobi column", j)


@pytest.mark.parametrize("colmode", [0, 1], ids=["col16", "col32"])
@pytest.mark.parametrize("k", ops.BLOCK_WIDTHS)
@pytest.mark.parametrize("name", SV.SELL_CASES)
def test_every_block_kernel_bit_exact(name, k, colmode):
    bp = block_problem(name)
    dA, S = twin(bp.A, colmode)
    for nt in SV.SELL_NTS:
        with SV.tuned(sell_nt=nt):
            check_block_sweeps((name, k, colmode, "sell_nt", nt), dA, S, bp, k)
            check_independence((name, k, colmode, "sell_nt", nt), S, bp, k)


@pytest.mark.parametrize("colmode", [0, 1], ids=["col16", "col32"])
@pytest.mark.parametrize("k", ops.BLOCK_WIDTHS)
@pytest.mark.parametrize("name", ["rect_tall", "rect_wide"])
def test_rectangular_block_spmv_bit_exact(name, k, colmode):
    bp = block_problem(name)
    dA, S = twin(bp.A, colmode)
    assert S.shape == ((77, 200) if name == "rect_wide" else (200, 77))
    assert S.max_len == 25 if name == "rect_wide" else 1 <= S.max_len <= 9
    for nt in SV.SELL_NTS:
        with SV.tuned(sell_nt=nt):
            check_block_spmv((name, k, colmode, "sell_nt", nt), S, bp, k)
            check_independence((name, k, colmode, "sell_nt", nt), S, bp, k)


def test_a_zero_column_stays_zero():
    bp = block_problem("ragged_slices")
    dA, S = twin(bp.A, 0)
    n = S.shape[0]
    X, B = bp.X[:, :4].copy(), bp.B[:, :4].copy()
    X[:, 3] = B[:, 3] = 0.0
    dX, dB = SV.dev(X), SV.dev(B)
    for run in (lambda o: ops.block_jacobi(S, dX, dB, 0.8, o), lambda o: ops.block_residual_norm2(S, dX, dB, o, None, None),
                lambda o: ops.block_spmv(S, dX, o, -0.5, 0.0)):
        Out = GuardedBlock(n, 4)
        run(Out.out)
        assert not Out.result("zero column")[:, 3].any()


def test_block_wrappers_check_their_blocks():
    bp = block_problem("short_9")
    dA, S = twin(bp.A, 0)
    n = S.shape[0]
    X, B, Out = blk(bp.X, 4), blk(bp.B, 4), torch.zeros((n, 4), dtype=F64, device=DEV)
    with pytest.raises(ValueError):
        ops.block_jacobi(S, X, B, 0.8, torch.zeros((n, 2), dtype=F64, device=DEV))         # two widths
    with pytest.raises(ValueError):
        ops.block_jacobi(S, X[:, :3].contiguous(), B[:, :3].contiguous(), 0.8, Out[:, :3].contiguous())   # no width of 3
    with pytest.raises(TypeError):
        ops.block_jacobi(S, X.t().contiguous().t(), B, 0.8, Out)                           # not contiguous
    with pytest.raises(ValueError):
        ops.block_jacobi(S, X[1:], B, 0.8, Out)                                            # rows
    with pytest.raises(ValueError):
        ops.block_jacobi(S, X.view(-1), B, 0.8, Out)                                       # a block is 2-D
    odd = torch.zeros(n * 4 + 1, dtype=F64, device=DEV)[1:].view(n, 4)
    with pytest.raises(ValueError, match="aligned"):
        ops.block_jacobi(S, odd, B, 0.8, Out)
    with pytest.raises(ops.LmgError):
        ops.block_jacobi(S, X, B, 0.8, X)                                                  # in place
    part, n2 = torch.zeros(ops.block_partials_count(n, 4), dtype=F64, device=DEV), torch.zeros(4, dtype=F64, device=DEV)
    assert part.numel() == 4                                                               # 130 rows: one workgroup, 4 sums
    for bad_part, bad_n2 in ((part[:3], n2), (part, n2[:3]), (part, None), (None, n2)):
        with pytest.raises(ValueError):
            ops.block_residual_norm2(S, X, B, None, bad_part, bad_n2)
    ops.block_residual_norm2(S, X, B, None, part, n2)
    assert (n2.cpu().numpy() > 0).all()
    assert not Out.any()
