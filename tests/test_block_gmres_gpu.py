"""GMRES.solve_many (-m gpu): flexible GMRES on blocks of right-hand sides on the device, for the unsymmetric operator and
the cycles CG.solve_many refuses, against krylov_ref.fgmres_ref column by column (tests/block_gmres_ref.py: the problem, the
references, the bound |got - want| <= RTOL want + ATOL track[0] whose premise tests/test_block_gmres_cpu.py asserts), and bit
for bit against itself: a column does not feel which block it is solved in, a graph replay is the eager run, and solve()
does not feel solve_many."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import block_gmres_ref as R                                          # noqa: E402
from krylov_ref import fgmres_ref                                    # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy                   # noqa: E402
from learnmultigrid_amd.solvers import GMRES                         # noqa: E402
from support import DEV                                              # noqa: E402

N_IT, M = R.ITERATIONS, R.RESTART
KW = dict(restart=M, precond_steps=R.STEPS, precond_omega=R.OMEGA)


@functools.lru_cache(maxsize=None)
def hierarchy():
    A, hier, _, _ = R.problem()
    H = Hierarchy(A, hier, DEV)
    assert H.sizes == [1089, 289, 81] and H.coarse.kind == "dense"
    return H


def solver():
    A, _, B, _ = R.problem()
    return GMRES(A, B[:, :1].copy())


def precond(shape):
    return {} if shape is None else dict(preconditioner=hierarchy(), precond_cycle_shape=shape)


@pytest.mark.parametrize("shape", ["V", "F", None])
@pytest.mark.parametrize("m", [1, 3, 5, 11])
def test_histories_and_solutions_match_the_reference_column_by_column(m, shape):
    _, _, B, _ = R.problem()
    wx, wt, _ = R.reference(shape)
    gm = solver()
    X, track = gm.solve_many(B[:, :m], max_iterations=N_IT, error=0.0, **precond(shape), **KW)
    assert X.shape == (B.shape[0], m) and list(gm.iterations_many) == [N_IT] * m
    R.close(track, wt[:, :m])
    R.close_x(X, wx[:, :m])


def test_columns_stop_at_their_own_iteration():
    _, _, _, Bs = R.problem()
    wx, wt, wi = R.reference("V", True, 50, R.STOP_ERROR)
    assert wi == R.STOP_COUNTS
    gm = solver()
    X, track = gm.solve_many(Bs, max_iterations=50, error=R.STOP_ERROR, **precond("V"), **KW)
    assert list(gm.iterations_many) == wi and track.shape == (max(wi) + 1, R.MMAX)
    for j, f in enumerate(wi):
        assert np.isfinite(track[:f + 1, j]).all() and np.isnan(track[f + 1:, j]).all()
        assert track[f, j] <= R.STOP_ERROR < track[f - 1, j]
    R.close(track, wt)
    R.close_x(X, wx)


def test_columns_with_nothing_to_do_and_max_iterations_in_mid_cycle():
    A, _, B, _ = R.problem()
    n = B.shape[0]
    xs = np.linalg.solve(A.toarray(), B[:, 2])
    error = 1e-9
    assert np.linalg.norm(B[:, 2] - A @ xs) <= error
    Bs = np.column_stack([B[:, 1], np.zeros(n), B[:, 2]])
    X0 = np.column_stack([np.zeros(n), np.zeros(n), xs])
    wx, wt, wi = fgmres_ref(A, B[:, 1], R.cycle_operator("V"), restart=M, max_iterations=6, error=error)
    gm = solver()
    X, track = gm.solve_many(Bs, max_iterations=6, error=error, initial_guess=X0, **precond("V"), **KW)
    assert list(gm.iterations_many) == [6, 0, 0] == [wi, 0, 0] and track.shape == (7, 3)
    assert not X[:, 1].any() and np.array_equal(X[:, 2], xs)             # the initial guesses bit for bit
    assert track[0, 1] == 0.0 and track[0, 2] <= error and np.isnan(track[1:, 1:]).all()
    R.close(track[:, :1], np.array(wt)[:, None])                         # (6 iterations of GMRES(4): the last cycle has two steps)
    R.close_x(X[:, :1], wx[:, None])
    X2, track2 = gm.solve_many(Bs[:, 1:], max_iterations=6, error=error, initial_guess=X0[:, 1:], **precond("V"), **KW)
    assert list(gm.iterations_many) == [0, 0] and track2.shape == (1, 2) and np.array_equal(X2, X0[:, 1:])


def same_column(alone, block, j):
    """The column solved alone against column j of a block: the solution and the history to the bit, NaN rows behind it."""
    (Xa, ta), (Xb, tb) = alone, block
    rows = ta.shape[0]
    return (np.array_equal(Xa[:, 0], Xb[:, j]) and np.array_equal(ta[:, 0], tb[:rows, j])
            and np.isnan(tb[rows:, j]).all())


@pytest.mark.parametrize("shape", ["V", None])
def test_a_column_does_not_feel_the_block_it_is_solved_in(shape):
    """Columns 1 and 9 of the scaled right-hand sides alone (width 2), inside 5 columns (width 8) and inside 11 (chunks of
    width 8 and 4), with a threshold the columns pass at different steps of different cycles: the recurrence of a column is
    its own, and so are its bits."""
    _, _, _, Bs = R.problem()
    gm = solver()
    kw = dict(KW, max_iterations=50, error=R.STOP_ERROR, **precond(shape)) if shape else dict(KW, max_iterations=12, error=1.0)
    eleven = gm.solve_many(Bs, **kw)
    assert len(set(gm.iterations_many.tolist())) > 2                  # the columns of a block do stop apart
    five = gm.solve_many(Bs[:, :5], **kw)
    one = gm.solve_many(Bs[:, 1:2], **kw)
    nine = gm.solve_many(Bs[:, 9:10], **kw)
    assert np.isfinite(one[1]).all() and one[1].shape[0] >= 5
    assert same_column(one, five, 1)
    assert same_column(one, eleven, 1)
    assert same_column(nine, eleven, 9)


def test_graph_replay_gives_the_bits_of_the_eager_run():
    _, _, _, Bs = R.problem()
    gm = solver()
    kw = dict(KW, max_iterations=50, error=R.STOP_ERROR, **precond("F"))
    Xe, te = gm.solve_many(Bs[:, :5], **kw)
    Xg, tg = gm.solve_many(Bs[:, :5], use_graph=True, **kw)
    assert np.array_equal(Xe, Xg) and np.array_equal(te, tg, equal_nan=True)
    Xg2, tg2 = gm.solve_many(Bs[:, :5], use_graph=True, **kw)                      # the cached graph
    assert np.array_equal(Xe, Xg2) and np.array_equal(te, tg2, equal_nan=True)


def test_solve_after_solve_many_is_unchanged_and_agrees_with_it():
    _, _, B, _ = R.problem()
    kw = dict(max_iterations=N_IT, error=1e-30, **precond("V"), **KW)
    fresh = solver()
    fresh.solve(**kw)
    gm = solver()
    X, track = gm.solve_many(B[:, :5], max_iterations=N_IT, error=0.0, **precond("V"), **KW)
    gm.solve(**kw)
    assert np.array_equal(gm.get_track_res(), fresh.get_track_res()) and np.array_equal(gm.get_solution(), fresh.get_solution())
    assert gm.get_iterations() == fresh.get_iterations() == N_IT
    # solve() on column 0 (the solver's own right-hand side) and solve_many on it: other kernels reduce the norms and sweep
    # the cycle, so this is agreement, not bits -- over the first two cycles, where a perturbation moves the history by
    # 2e-11 relative and a relative comparison still holds (the rows behind them: the two-term bound)
    np.testing.assert_allclose(gm.get_track_res()[:2 * M + 1, 0], track[:2 * M + 1, 0], rtol=1e-8, atol=0)
    R.close(gm.get_track_res()[:, :1], track[:, :1])


def test_refusals():
    A, hier, B, _ = R.problem()
    gm = solver()
    with pytest.raises(ValueError, match="cycle_values"):
        gm.solve_many(B[:, :2], preconditioner=Hierarchy(A, hier, DEV, cycle_values="f32"))
    with pytest.raises(TypeError):
        gm.solve_many(B[:, :2], preconditioner=hierarchy(), precond_smoother="GaussSeidel")
    with pytest.raises(ValueError, match="restart"):
        gm.solve_many(B[:, :2], restart=65)
    with pytest.raises(ValueError, match="cycle shape"):
        gm.solve_many(B[:, :2], preconditioner=hierarchy(), precond_cycle_shape="X")
