"""CG.solve_many (-m gpu): multigrid-preconditioned conjugate gradients on blocks of right-hand sides on the device, against
the textbook recurrence in NumPy (tests/block_cg_ref.py: the problem, pcg_ref, the premise of the 1e-10 tolerance -- asserted
in tests/test_block_cg_cpu.py), and bit for bit against itself: a column does not feel which block it is solved in, a graph
replay is the eager run, and solve() does not feel solve_many."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import block_cg_ref as R                                             # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy                   # noqa: E402
from learnmultigrid_amd.solvers import CG                            # noqa: E402
from support import DEV                                              # noqa: E402

N_IT = R.ITERATIONS
KW = dict(precond_steps=R.STEPS, precond_omega=R.OMEGA)


@functools.lru_cache(maxsize=None)
def hierarchy():
    A, hier, _ = R.problem()
    H = Hierarchy(A, hier, DEV)
    assert H.sizes == [1089, 289, 81] and H.coarse.kind == "dense"
    return H


def solver():
    A, _, B = R.problem()
    return CG(A, B[:, :1].copy())


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=R.RTOL, atol=0)


def close_x(got, want):
    np.testing.assert_allclose(got, want, rtol=R.RTOL, atol=R.RTOL * np.abs(want).max())


@pytest.mark.parametrize("m", [1, 3, 5, 11])
def test_histories_and_solutions_match_the_recurrence_column_by_column(m):
    _, _, B = R.problem()
    wt, wx = R.reference("V")
    cg = solver()
    X, track = cg.solve_many(B[:, :m], max_iterations=N_IT, error=0.0, preconditioner=hierarchy(), **KW)
    assert X.shape == (B.shape[0], m) and track.shape == (N_IT + 1, m) and list(cg.iterations_many) == [N_IT] * m
    close(track, wt[:N_IT + 1, :m])
    close_x(X, wx[N_IT][:, :m])


def test_w_cycle_preconditioner():
    _, _, B = R.problem()
    wt, wx = R.reference("W", N_IT, 3)
    X, track = solver().solve_many(B[:, :3], max_iterations=N_IT, error=0.0, preconditioner=hierarchy(),
                                   precond_cycle_shape="W", **KW)
    close(track, wt)
    close_x(X, wx[N_IT])


def test_refusals():
    A, hier, B = R.problem()
    cg = solver()
    with pytest.raises(ValueError, match="symmetric"):
        cg.solve_many(B[:, :2], preconditioner=hierarchy(), precond_cycle_shape="F")
    with pytest.raises(ValueError, match="cycle_values"):
        cg.solve_many(B[:, :2], preconditioner=Hierarchy(A, hier, DEV, cycle_values="f32"))
    with pytest.raises(TypeError):
        cg.solve_many(B[:, :2], preconditioner=hierarchy(), precond_smoother="GaussSeidel")


def test_without_a_preconditioner():
    _, _, B = R.problem()
    wt, wx = R.reference(None, 14, 3)
    cg = solver()
    X, track = cg.solve_many(B[:, :3], max_iterations=10, error=0.0)
    assert track.shape == (11, 3) and list(cg.iterations_many) == [10] * 3
    close(track, wt[:11])
    close_x(X, wx[10])


def test_a_column_freezes_at_the_iteration_it_passes():
    _, _, B = R.problem()
    cols, error = [0, 1, 9], 1e-7
    wt, wx = R.reference("V")
    first = R.first_pass(wt[:, cols], error)
    assert first == [6, 8, 7]
    cg = solver()
    X, track = cg.solve_many(B[:, cols], max_iterations=50, error=error, preconditioner=hierarchy(), **KW)
    assert list(cg.iterations_many) == first and track.shape == (max(first) + 1, 3)
    for c, (j, f) in enumerate(zip(cols, first)):
        close(track[:f + 1, c], wt[:f + 1, j])
        assert track[f, c] <= error < track[f - 1, c] and np.isnan(track[f + 1:, c]).all()
        close_x(X[:, c], wx[f][:, j])
    # the frozen solution is the iterate of that iteration, bit for bit: the same columns stopped there by max_iterations
    for c, f in enumerate(first):
        Xf, _ = cg.solve_many(B[:, cols], max_iterations=f, error=error, preconditioner=hierarchy(), **KW)
        assert np.array_equal(Xf[:, c], X[:, c])


def test_chunks_of_different_length_and_columns_with_nothing_to_do():
    A, _, B = R.problem()
    wt, wx = R.reference("V")
    error = 1e-5
    first = R.first_pass(wt, error)
    n = B.shape[0]
    xs = np.linalg.solve(A.toarray(), B[:, 2])
    assert np.linalg.norm(B[:, 2] - A @ xs) <= error
    # a chunk of 8 slow columns, then one of three: a fast one, a zero right-hand side, an initial guess that solves it
    Bs = np.column_stack([B[:, 1:9], B[:, 0], np.zeros(n), B[:, 2]])
    X0 = np.zeros_like(Bs)
    X0[:, 10] = xs
    cg = solver()
    X, track = cg.solve_many(Bs, max_iterations=50, error=error, initial_guess=X0, preconditioner=hierarchy(), **KW)
    assert list(cg.iterations_many) == first[1:9] + [first[0], 0, 0]
    rows8, rows3 = max(first[1:9]) + 1, first[0] + 1
    assert rows3 < rows8 and track.shape == (rows8, 11)
    close(track[:, :8], np.where(np.arange(rows8)[:, None] <= np.array(first[1:9])[None, :], wt[:rows8, 1:9], np.nan))
    close(track[:rows3, 8], wt[:rows3, 0])
    assert np.isnan(track[rows3:, 8:]).all() and np.isnan(track[1:, 9:]).all()
    assert track[0, 9] == 0.0 and track[0, 10] <= error
    assert np.isfinite(X).all() and not X[:, 9].any() and np.array_equal(X[:, 10], xs)
    for c in range(8):
        close_x(X[:, c], wx[first[1 + c]][:, 1 + c])
    close_x(X[:, 8], wx[first[0]][:, 0])


def same_column(alone, block, j):
    """The column solved alone against column j of a block: the solution and the history to the bit, NaN rows behind it."""
    (Xa, ta), (Xb, tb) = alone, block
    rows = ta.shape[0]
    return (np.array_equal(Xa[:, 0], Xb[:, j]) and np.array_equal(ta[:, 0], tb[:rows, j])
            and np.isnan(tb[rows:, j]).all())


@pytest.mark.parametrize("precond", [True, False])
def test_a_column_does_not_feel_the_block_it_is_solved_in(precond):
    """Columns 1 and 9 alone (width 2), inside 5 columns (width 8) and inside 11 (chunks of width 8 and 4), with a
    threshold the columns pass at different iterations: per-column scalars, so the bits of a column are its own."""
    _, _, B = R.problem()
    cg = solver()
    kw = dict(KW, preconditioner=hierarchy(), max_iterations=50, error=1e-7) if precond else dict(max_iterations=12, error=1.0)
    eleven = cg.solve_many(B, **kw)
    assert len(set(cg.iterations_many.tolist())) > 1                  # the columns of a block do stop apart
    five = cg.solve_many(B[:, :5], **kw)
    one = cg.solve_many(B[:, 1:2], **kw)
    nine = cg.solve_many(B[:, 9:10], **kw)
    assert np.isfinite(one[1]).all() and one[1].shape[0] >= 8
    assert same_column(one, five, 1)
    assert same_column(one, eleven, 1)
    assert same_column(nine, eleven, 9)


def test_graph_replay_gives_the_bits_of_the_eager_run():
    _, _, B = R.problem()
    cg = solver()
    kw = dict(KW, preconditioner=hierarchy(), max_iterations=50, error=1e-7)
    Xe, te = cg.solve_many(B[:, :5], **kw)
    Xg, tg = cg.solve_many(B[:, :5], use_graph=True, **kw)
    assert np.array_equal(Xe, Xg) and np.array_equal(te, tg, equal_nan=True)
    Xg2, tg2 = cg.solve_many(B[:, :5], use_graph=True, **kw)                       # the cached graph
    assert np.array_equal(Xe, Xg2) and np.array_equal(te, tg2, equal_nan=True)


def test_solve_after_solve_many_is_unchanged():
    _, _, B = R.problem()
    kw = dict(max_iterations=6, error=1e-30, preconditioner=hierarchy(), **KW)
    fresh = solver()
    fresh.solve(**kw)
    cg = solver()
    cg.solve_many(B[:, :5], max_iterations=3, error=0.0, preconditioner=hierarchy(), **KW)
    cg.solve(**kw)
    assert np.array_equal(cg.get_track_res(), fresh.get_track_res()) and np.array_equal(cg.get_solution(), fresh.get_solution())
    assert cg.get_iterations() == fresh.get_iterations() == 6
    wt, _ = R.reference("V")
    np.testing.assert_allclose(cg.get_track_res()[:, 0], wt[:7, 0], rtol=1e-8, atol=0)   # (other kernels: agreement, not bits)
