"""Conjugate gradients on blocks of right-hand sides without a GPU: the argument rules of the three entry points (through
ctypes, where every refusal comes before any HIP call), and the host logic of krylov.block_pcg / block_pcg_columns on
NumPy stand-ins of the block ops (tests/block_cg_ref.py) -- padding, chunking, per-column scalars, freezing -- against the
textbook recurrence pcg_ref run column by column with the oracle's cycle as the preconditioner.

The tolerance is the project's for histories, 1e-10 relative, after 8 iterations: PCG contracts by 0.05 .. 0.08 per
iteration here, every column is at 2e-9 .. 3e-10 of its start then, nothing has reached a floor, and the order of the
sums moves the history by parts in 1e-14 (test_the_premise_*), four orders below."""
import numpy as np
import pytest

import block_cg_ref as R
import cpu_ops_shim as shim
from learnmultigrid_amd import _lib, krylov
from learnmultigrid_amd.block import BlockCycle, block_width
from learnmultigrid_amd.hierarchy import Hierarchy
from learnmultigrid_amd.solvers import CG

OK, ERR_ARG, ERR_ALIGN = 0, -1, -2
N_IT = R.ITERATIONS


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


BAD_WIDTHS = (0, 1, 3, 5, 6, 7, 16, -2)


def test_block_dot_refuses_before_any_launch(L):
    n = 64
    X, Y, part, out = aligned(n * 8), aligned(n * 8), aligned(1024 * 8), aligned(8)
    for k in BAD_WIDTHS:
        assert L.lmg_block_dot(k, n, p(X), p(Y), p(part), p(out), None) == ERR_ARG, k
        assert L.lmg_block_dot(k, 0, None, None, None, None, None) == ERR_ARG           # the width is checked first
    for k in R.WIDTHS:
        assert L.lmg_block_dot_partials_count(n, k) == 1024 * k
        assert L.lmg_block_dot_partials_count(2 ** 31 + 7, k) == 1024 * k               # fixed geometry
        assert L.lmg_block_dot(k, 0, None, None, None, None, None) == OK                # n == 0: nothing to do
        assert L.lmg_block_dot(k, -1, p(X), p(Y), p(part), p(out), None) == ERR_ARG
        for hole in range(4):
            args = [p(X), p(Y), p(part), p(out)]
            args[hole] = None
            assert L.lmg_block_dot(k, n, *args, None) == ERR_ARG, hole
        X8 = aligned(n * 8, 8)
        assert L.lmg_block_dot(k, n, p(X8), p(Y), p(part), p(out), None) == ERR_ALIGN
        assert L.lmg_block_dot(k, n, p(X), p(X8), p(part), p(out), None) == ERR_ALIGN
    assert not part.any() and not out.any()


def test_block_cg_step_refuses_before_any_launch(L):
    n = 64
    rz, pAp, tol2, mask, rr = (aligned(8) for _ in range(5))
    Pb, AP, X, Rb = (aligned(n * 8) for _ in range(4))
    part = aligned(1024 * 8)

    def step(k, n_=n, **over):
        a = dict(rz=rz, pAp=pAp, tol2=tol2, mask=mask, P=Pb, AP=AP, X=X, R=Rb, part=part, rr=rr)
        a.update(over)
        return L.lmg_block_cg_step(k, n_, *(p(a[name]) for name in ("rz", "pAp", "tol2", "mask", "P", "AP", "X", "R", "part", "rr")),
                                   None)

    for k in BAD_WIDTHS:
        assert step(k) == ERR_ARG, k
        assert step(k, 0) == ERR_ARG
    for k in R.WIDTHS:
        assert step(k, 0) == OK
        assert step(k, -1) == ERR_ARG
        for name in ("rz", "pAp", "tol2", "mask", "P", "AP", "X", "R", "part", "rr"):
            assert step(k, **{name: None}) == ERR_ARG, name
        assert step(k, X=Pb) == ERR_ARG                                                 # x = alpha p + x in place of p
        assert step(k, R=AP) == ERR_ARG
        assert step(k, X=Rb) == ERR_ARG and step(k, X=AP) == ERR_ARG and step(k, R=Pb) == ERR_ARG
        assert step(k, rr=rz) == ERR_ARG and step(k, rr=pAp) == ERR_ARG and step(k, rr=mask) == ERR_ARG
        for name in ("P", "AP", "X", "R"):
            assert step(k, **{name: aligned(n * 8, 8)}) == ERR_ALIGN, name
    assert not X.any() and not Rb.any() and not rr.any() and not mask.any() and not part.any()


def test_block_cg_direction_refuses_before_any_launch(L):
    n = 64
    rz_new, rz_old, mask = aligned(8), aligned(8), aligned(8)
    Z, Pb = aligned(n * 8), aligned(n * 8)

    def direction(k, n_=n, **over):
        a = dict(rz_new=rz_new, rz_old=rz_old, mask=mask, Z=Z, P=Pb)
        a.update(over)
        return L.lmg_block_cg_direction(k, n_, *(p(a[name]) for name in ("rz_new", "rz_old", "mask", "Z", "P")), None)

    for k in BAD_WIDTHS:
        assert direction(k) == ERR_ARG, k
        assert direction(k, 0) == ERR_ARG
    for k in R.WIDTHS:
        assert direction(k, 0) == OK
        assert direction(k, -1) == ERR_ARG
        for name in ("rz_new", "rz_old", "mask", "Z", "P"):
            assert direction(k, **{name: None}) == ERR_ARG, name
        assert direction(k, P=Z) == ERR_ARG
        assert direction(k, rz_new=rz_old) == ERR_ARG                                   # the driver alternates between two arrays
        assert direction(k, Z=aligned(n * 8, 8)) == ERR_ALIGN
        assert direction(k, P=aligned(n * 8, 8)) == ERR_ALIGN
    assert not Pb.any()


# ---- the premise of the tolerance ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,iterations", [("V", N_IT), (None, 10)])
def test_the_premise_summation_order_moves_the_history_by_less_than_1e_12(shape, iterations):
    A, _, B = R.problem()
    M = None if shape is None else R.cycle_operator(shape)
    for j in (0, 1):
        a, Xa = R.pcg_ref(A, B[:, j], M, iterations)
        b, Xb = R.pcg_ref(A, B[:, j], M, iterations, dot=R.dot_reversed)
        assert not np.array_equal(a, b)                                  # the orders do differ
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
        np.testing.assert_allclose(Xa[-1], Xb[-1], rtol=1e-12, atol=1e-12 * np.abs(Xb[-1]).max())
    if shape == "V":
        track, _ = R.reference("V")
        ratio = track[2:N_IT + 1] / track[1:N_IT]
        assert 0.04 < ratio.min() and ratio.max() < 0.1                  # contracts by 0.05 .. 0.08 per iteration
        assert (track[N_IT] < 3e-9 * track[0]).all() and (track[N_IT] > 1e-10 * track[0]).all()


# ---- the driver on the stand-ins ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup():
    A, hier, B = R.problem()
    H = Hierarchy(A, hier, "cpu", ops_mod=R.block_namespace(shim))
    assert H.sizes == [1089, 289, 81] and H.coarse.kind == "dense"
    return H, B


def run(H, B, X0=None, precond=True, **kw):
    """What CG.solve_many does below its keyword checks."""
    seen = []

    def block_cycle(mc):
        seen.append(mc)
        if not precond:
            return None
        bc = BlockCycle(H, mc)
        assert bc.k == block_width(mc, R.WIDTHS)
        return bc

    kw = dict(dict(max_iterations=N_IT, error=0.0, steps=R.STEPS, omega=R.OMEGA), **kw)
    X, track, its = krylov.block_pcg_columns(H.ops, H.levels[0].A, block_cycle, np.asarray(B), X0, "cpu", **kw)
    assert seen == [min(8, B.shape[1] - c0) for c0 in range(0, B.shape[1], 8)]          # chunks of 8, then the rest
    return X, track, its


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=R.RTOL, atol=0)


def close_x(got, want):
    np.testing.assert_allclose(got, want, rtol=R.RTOL, atol=R.RTOL * np.abs(want).max())


@pytest.mark.parametrize("m", [1, 3, 5, 11])
def test_histories_and_solutions_match_the_recurrence_column_by_column(setup, m):
    H, B = setup
    wt, wx = R.reference("V")
    X, track, its = run(H, B[:, :m])                  # (block_pcg_columns raises if a padding column left zero)
    assert X.shape == (B.shape[0], m) and track.shape == (N_IT + 1, m) and list(its) == [N_IT] * m
    close(track, wt[:N_IT + 1, :m])
    close_x(X, wx[N_IT][:, :m])


def test_w_cycle_preconditioner(setup):
    H, B = setup
    wt, wx = R.reference("W", N_IT, 3)
    vt, _ = R.reference("V")
    assert (np.abs(wt[N_IT] / vt[N_IT, :3] - 1.0) > 1e-6).any()          # the shapes are told apart
    X, track, _ = run(H, B[:, :3], shape="W")
    close(track, wt)
    close_x(X, wx[N_IT])


def test_f_cycle_is_refused_with_the_message_of_solve():
    A, _, B = R.problem()
    cg = CG(A, B[:, :1].copy(), device="cpu")
    with pytest.raises(ValueError) as single:
        cg.solve(precond_cycle_shape="F")
    with pytest.raises(ValueError) as many:
        cg.solve_many(B[:, :2], precond_cycle_shape="F")
    assert str(many.value) == str(single.value) and "symmetric" in str(many.value)
    for rhs in (B[:, 0], B[:-1, :2], np.zeros((B.shape[0], 0))):
        with pytest.raises(ValueError, match="rhs"):
            cg.solve_many(rhs)
    with pytest.raises(ValueError, match="initial_guess"):
        cg.solve_many(B[:, :2], initial_guess=B[:, :3])
    with pytest.raises(TypeError):
        cg.solve_many(B[:, :2], precond_smoother="GaussSeidel")          # the keyword is not offered


def test_without_a_preconditioner(setup):
    H, B = setup
    wt, wx = R.reference(None, 14, 3)
    X, track, its = run(H, B[:, :3], precond=False, max_iterations=10)
    assert track.shape == (11, 3) and list(its) == [10] * 3
    close(track, wt[:11])
    close_x(X, wx[10])


def test_a_column_freezes_at_the_iteration_it_passes(setup):
    H, B = setup
    cols, error = [0, 1, 9], 1e-7
    wt, wx = R.reference("V")
    first = R.first_pass(wt[:, cols], error)
    assert first == [6, 8, 7]                                            # three columns, three different iterations
    X, track, its = run(H, B[:, cols], max_iterations=50, error=error)
    assert list(its) == first
    assert track.shape == (max(first) + 1, 3)                            # the loop ends with the slowest column
    for c, (j, f) in enumerate(zip(cols, first)):
        close(track[:f + 1, c], wt[:f + 1, j])
        assert track[f, c] <= error < track[f - 1, c]
        assert np.isnan(track[f + 1:, c]).all()                          # nothing is recorded for a frozen column
        close_x(X[:, c], wx[f][:, j])                                    # the iterate of iteration f, not of a later one
        assert not np.allclose(X[:, c], wx[max(first)][:, j], rtol=1e-13, atol=0) or f == max(first)


def test_chunks_of_different_length_leave_nan_rows(setup):
    H, B = setup
    wt, _ = R.reference("V")
    error = 1e-5
    first = R.first_pass(wt, error)
    assert max(first[1:9]) == 6 and first[0] == 4
    Bs = np.column_stack([B[:, 1:9], B[:, 0], B[:, 0]])                  # 8 slow columns, then a chunk of two fast ones
    X, track, its = run(H, Bs, max_iterations=50, error=error)
    assert list(its) == first[1:9] + [4, 4] and track.shape == (7, 10)
    close(track[:, :8], wt[:7, 1:9])
    close(track[:5, 8], wt[:5, 0])
    assert np.isnan(track[5:, 8:]).all()
    assert np.array_equal(X[:, 8], X[:, 9])


def test_columns_with_nothing_to_do_run_no_iteration(setup):
    H, B = setup
    A = R.problem()[0]
    wt, wx = R.reference("V")
    xs = np.linalg.solve(A.toarray(), B[:, 2])
    Bs = np.column_stack([B[:, 1], np.zeros(B.shape[0]), B[:, 2]])
    X0 = np.column_stack([np.zeros(B.shape[0]), np.zeros(B.shape[0]), xs])
    error = 1e-9
    assert np.linalg.norm(B[:, 2] - A @ xs) <= error
    X, track, its = run(H, Bs, X0=X0, max_iterations=4, error=error)
    assert list(its) == [4, 0, 0] and track.shape == (5, 3)
    assert np.isfinite(X).all() and not X[:, 1].any() and np.array_equal(X[:, 2], xs)
    assert track[0, 1] == 0.0 and track[0, 2] <= error and np.isnan(track[1:, 1:]).all()
    close(track[:, 0], wt[:5, 1])
    close_x(X[:, 0], wx[4][:, 1])
    # all columns done at the start: no iteration at all, X is the initial guess
    X2, track2, its2 = run(H, Bs[:, 1:], X0=X0[:, 1:], max_iterations=4, error=error)
    assert list(its2) == [0, 0] and track2.shape == (1, 2) and np.array_equal(X2, X0[:, 1:])
