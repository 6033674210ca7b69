"""The multi-right-hand-side path without a GPU: the argument rules of the three block entry points (through ctypes, where
every refusal comes before any HIP call), and the host logic of block.BlockCycle on a NumPy stand-in of the block ops --
padding, chunking, the recursion of the three cycle shapes -- against the CPU restatements of the cycle."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import block_cg_ref
import cpu_ops_shim as shim
from cycle_shapes_ref import ShapeCycle
from learnmultigrid_amd import _lib, problems as P
from learnmultigrid_amd.block import BlockCycle, block_width
from learnmultigrid_amd.hierarchy import Hierarchy
from learnmultigrid_amd.solvers import HierarchyMG
from oracle.vcycle_ref import HoistedVCycle

OK, ERR_ARG, ERR_ALIGN = 0, -1, -2
WIDTHS = (2, 4, 8)


# ---- the C entry points -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    _lib.build()
    lib = _lib.lib()
    if lib.lmg_device_count() > 0:
        pytest.skip("a device is visible: host pointers are not handed to entry points that could launch on it")
    return lib


def aligned(n, off=0):
    """n doubles that start `off` bytes behind a 16-byte boundary (the array keeps its buffer alive)."""
    buf = np.zeros(n + 4)
    start = ((off - buf.ctypes.data) % 16) // 8
    a = buf[start:start + n]
    assert a.ctypes.data % 16 == off
    return a


def p(a):
    return None if a is None else a.ctypes.data


def sell_args(n=64):
    """Host arrays with the shapes of a one-slice SELL twin (never read: every call below is refused first)."""
    return dict(sb=np.zeros(1, dtype=np.int64), sl=np.ones(1, dtype=np.int32), cm=np.zeros(1, dtype=np.int32),
                rl=np.ones(n, dtype=np.int32), col=np.zeros(128, dtype=np.int32), val=aligned(128))


def sweep(L, mode, k, n, s, X, B, Out, part=None, n2=None, colmode=1, max_len=1, **drop):
    a = dict(s, **drop)
    return L.lmg_sell_sweep_block(mode, k, n, p(a["sb"]), p(a["sl"]), p(a["cm"]), p(a["rl"]), p(a["col"]), colmode, p(a["val"]),
                                  max_len, p(X), p(B), p(Out), 0.8, 0.0, p(part), p(n2), None)


def test_block_sweep_refuses_before_any_launch(L):
    s, n = sell_args(), 64
    X, B, Out, part, n2 = aligned(n * 8), aligned(n * 8), aligned(n * 8), aligned(64), aligned(8)
    for k in (0, 1, 3, 5, 6, 7, 16, -2):
        for mode in (0, 1, 2):
            assert sweep(L, mode, k, n, s, X, B, Out, part, n2) == ERR_ARG, (k, mode)
        assert sweep(L, 1, k, 0, s, X, B, Out) == ERR_ARG                      # the width is checked first, even for n == 0
    for k in WIDTHS:
        assert sweep(L, 1, k, 0, s, None, None, None) == OK                    # n == 0: nothing to do
        assert sweep(L, 1, k, -1, s, X, B, Out) == ERR_ARG
        assert sweep(L, 3, k, n, s, X, B, Out) == ERR_ARG                      # no such mode
        assert sweep(L, 1, k, n, s, X, B, Out, colmode=2) == ERR_ARG
        for name in ("sb", "sl", "rl", "col", "val"):
            assert sweep(L, 1, k, n, s, X, B, Out, **{name: None}) == ERR_ARG, name
        assert sweep(L, 1, k, n, s, X, B, Out, colmode=0, cm=None) == ERR_ARG   # uint16 columns need the slice bases
        assert sweep(L, 1, k, n, s, None, B, Out) == ERR_ARG
        assert sweep(L, 1, k, n, s, X, None, Out) == ERR_ARG                    # Jacobi: b and out
        assert sweep(L, 1, k, n, s, X, B, None) == ERR_ARG
        assert sweep(L, 1, k, n, s, X, B, X) == ERR_ARG                         # not in place
        assert sweep(L, 2, k, n, s, X, None, X) == ERR_ARG
        assert sweep(L, 2, k, n, s, X, None, None) == ERR_ARG
        assert sweep(L, 0, k, n, s, X, None, Out, part, n2) == ERR_ARG          # residual: b
        assert sweep(L, 0, k, n, s, X, B, Out, part, None) == ERR_ARG           # partials and norm2 come together
        assert sweep(L, 0, k, n, s, X, B, None, None, None) == ERR_ARG          # neither r nor a norm: nothing asked
        X8, B8, O8 = aligned(n * 8, 8), aligned(n * 8, 8), aligned(n * 8, 8)
        assert sweep(L, 1, k, n, s, X8, B, Out) == ERR_ALIGN
        assert sweep(L, 1, k, n, s, X, B8, Out) == ERR_ALIGN
        assert sweep(L, 1, k, n, s, X, B, O8) == ERR_ALIGN
        assert sweep(L, 2, k, n, s, X8, None, Out) == ERR_ALIGN
        assert sweep(L, 0, k, n, s, X, B8, None, part, n2) == ERR_ALIGN
    assert not Out.any() and not part.any() and not n2.any()


def test_dense_gemv_block_refuses_before_any_launch(L):
    M, X, Y = aligned(6 * 4), aligned(4 * 8), aligned(6 * 8)
    for k in (0, 1, 3, 6, 16):
        assert L.lmg_dense_gemv_block(k, 6, 4, p(M), p(X), p(Y), None) == ERR_ARG
        assert L.lmg_dense_gemv_block(k, 0, 4, None, None, None, None) == ERR_ARG
    for k in WIDTHS:
        assert L.lmg_dense_gemv_block(k, 0, 4, None, None, None, None) == OK
        assert L.lmg_dense_gemv_block(k, -1, 4, p(M), p(X), p(Y), None) == ERR_ARG
        assert L.lmg_dense_gemv_block(k, 6, -1, p(M), p(X), p(Y), None) == ERR_ARG
        assert L.lmg_dense_gemv_block(k, 6, 4, None, p(X), p(Y), None) == ERR_ARG
        assert L.lmg_dense_gemv_block(k, 6, 4, p(M), None, p(Y), None) == ERR_ARG
        assert L.lmg_dense_gemv_block(k, 6, 4, p(M), p(X), None, None) == ERR_ARG
        assert L.lmg_dense_gemv_block(k, 6, 4, p(M), p(X), p(X), None) == ERR_ARG
        assert L.lmg_dense_gemv_block(k, 6, 4, p(aligned(24, 8)), p(X), p(Y), None) == ERR_ALIGN
        assert L.lmg_dense_gemv_block(k, 6, 4, p(M), p(aligned(32, 8)), p(Y), None) == ERR_ALIGN
        assert L.lmg_dense_gemv_block(k, 6, 4, p(M), p(X), p(aligned(48, 8)), None) == ERR_ALIGN
    assert not Y.any()


def test_block_partials_count_covers_every_workgroup():
    _lib.build()
    lib = _lib.lib()
    for n in (0, 1, 64, 255, 256, 257, 1089, 2049 * 2049, 2 ** 31 - 200):
        nblocks = ((n + 63) // 64 + 3) // 4                   # four slices of 64 rows per workgroup (csrc/sell.hip)
        for k in WIDTHS:
            assert lib.lmg_block_partials_count(n, k) >= max(nblocks, 1) * k, (n, k)


# ---- the driver on a NumPy stand-in ---------------------------------------------------------------------------------------
def block_namespace():
    """cpu_ops_shim.namespace() plus the block sweeps on (n, k) CPU tensors, block_cg_ref's stand-ins: a "twin" is the matrix
    itself.  No Krylov op: the package reads an absent name as "not offered"."""
    return shim.namespace(BLOCK_WIDTHS=WIDTHS, block_twin=lambda A: A, block_partials_count=lambda n, k: (n // 256 + 1) * k,
                          block_residual_norm2=block_cg_ref.block_residual_norm2, block_jacobi=block_cg_ref.block_jacobi,
                          block_spmv=block_cg_ref.block_spmv, dense_gemv_block=block_cg_ref.dense_gemv_block)


def learned_like_hierarchy(side, levels, seed=43):
    hier = []
    for l, s in enumerate(P.level_sizes(side, levels)[:-1]):
        base = sp.kron(P.pseudo_l2_interpolator_1d(s), P.pseudo_l2_interpolator_1d(s)).tocsr()
        hier.append(P.learned_like(base, seed + l))
    return hier


CYCLES = 5


@pytest.fixture(scope="module")
def problem():
    """The 33^2 jittered problem on 3 levels, 11 right-hand sides (column 0: its own), and per cycle shape the reference
    histories and iterates of every column -- computed once."""
    A, rhs = P.jittered_poisson_2d(32, seed=42)
    hier = learned_like_hierarchy(33, 3)
    B = np.column_stack([rhs.ravel(), np.random.default_rng(5).standard_normal((A.shape[0], 10))])
    want = {}
    for shape in ("V", "W", "F"):
        ref = HoistedVCycle(A, hier) if shape == "V" else ShapeCycle(A, hier, shape)
        hist, Xw = np.empty((CYCLES + 1, 11)), np.empty_like(B)
        for j in range(11):
            x = np.zeros(A.shape[0])
            for it in range(CYCLES):
                hist[it, j] = np.linalg.norm(B[:, j] - A @ x)
                x = ref.cycle(x, B[:, j], "Jacobi", 2, 0.8)
            hist[CYCLES, j] = np.linalg.norm(B[:, j] - A @ x)
            Xw[:, j] = x
        want[shape] = (hist, Xw)
    H = Hierarchy(A, hier, "cpu", ops_mod=block_namespace())
    assert H.sizes == [1089, 289, 81] and H.coarse.kind == "dense"
    return A, B, H, want


def run_columns(H, B, shape):
    """What solve_many does above the cycle: chunks of 8 columns, each padded to the next width."""
    hist, X = np.empty((CYCLES + 1, B.shape[1])), np.empty_like(B)
    for c0 in range(0, B.shape[1], 8):
        mc = min(8, B.shape[1] - c0)
        bc = BlockCycle(H, mc)
        assert bc.k == block_width(mc, WIDTHS) and bc.levels[0].x.shape == (B.shape[0], bc.k)
        bc.levels[0].b[:, :mc] = torch.from_numpy(np.ascontiguousarray(B[:, c0:c0 + mc]))
        for it in range(CYCLES):
            hist[it, c0:c0 + mc] = bc.residual_norms()
            bc.cycle(2, 0.8, shape)
        hist[CYCLES, c0:c0 + mc] = bc.residual_norms()
        X[:, c0:c0 + mc] = bc.levels[0].x[:, :mc].numpy()
        assert not bc.levels[0].x[:, mc:].any()                                # a zero column stays zero
    return hist, X


@pytest.mark.parametrize("shape", ["V", "W", "F"])
@pytest.mark.parametrize("m", [1, 3, 5, 11])
def test_block_cycle_reproduces_the_single_vector_histories(problem, m, shape):
    A, B, H, want = problem
    hist, X = run_columns(H, B[:, :m], shape)
    wh, wx = want[shape]
    assert (wh[-1] < 1e-2 * wh[0]).all()                                  # the cycles converge: the histories say something
    np.testing.assert_allclose(hist, wh[:, :m], rtol=1e-10, atol=0)
    np.testing.assert_allclose(X, wx[:, :m], rtol=1e-10, atol=1e-10 * np.abs(wx).max())


def test_block_widths():
    assert [block_width(m, WIDTHS) for m in range(1, 10)] == [2, 2, 4, 4, 8, 8, 8, 8, 8]


def test_block_cycle_refusals(problem):
    A, B, H, _ = problem
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            BlockCycle(H, bad)
    bc = BlockCycle(H, 3)
    with pytest.raises(ValueError):
        bc.cycle(2, 0.8, "X")
    with pytest.raises(ValueError):
        bc.use_columns(2)                                                      # another width: another BlockCycle
    H.cycle_values = "f32"
    try:
        with pytest.raises(ValueError, match="cycle_values"):
            BlockCycle(H, 3)
    finally:
        H.cycle_values = "f64"


def test_solve_many_checks_its_keywords_before_any_setup(problem):
    A, B, _, _ = problem
    mg = HierarchyMG(A, B[:, :1].copy(), learned_like_hierarchy(33, 3), device="cpu")
    n = A.shape[0]
    for rhs in (B[:, 0], B[:n - 1, :2], np.zeros((n, 0)), B.T):
        with pytest.raises(ValueError, match="rhs"):
            mg.solve_many(rhs, levels=3)
    with pytest.raises(ValueError, match="cycle shape"):
        mg.solve_many(B[:, :2], levels=3, cycle_shape="X")
    with pytest.raises(ValueError, match="levels"):
        mg.solve_many(B[:, :2], levels=1)
    with pytest.raises(ValueError, match="Jacobi"):
        mg.solve_many(B[:, :2], levels=3, smoother="GaussSeidel")
    with pytest.raises(ValueError, match="initial_guess"):
        mg.solve_many(B[:, :2], levels=3, initial_guess=B[:, :3])
    assert mg._hier is None                                                     # nothing was set up
