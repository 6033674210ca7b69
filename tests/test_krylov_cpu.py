"""Restarted flexible GMRES without a GPU: the NumPy twin (tests/krylov_ref.py) against SciPy's GMRES, the product's
iteration (learnmultigrid_amd/krylov.py) on the ops shim against the twin, flexibility (a preconditioner that changes from
step to step), optimality against the stationary iteration, the edge cases, and the keyword checks of solvers.GMRES."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import cpu_ops_shim as shim
from krylov_ref import fgmres_ref
from learnmultigrid_amd import krylov
from learnmultigrid_amd import problems as P
from learnmultigrid_amd.ops import DeviceCSR
from learnmultigrid_amd.solvers.GMRES import check_keywords


def jacobi_M(A, sweeps, omega=0.8):
    """z = `sweeps` damped Jacobi sweeps on A z = v from zero: a fixed linear operator."""
    dinv = 1.0 / A.diagonal()

    def M(v):
        z = np.zeros_like(v)
        for _ in range(sweeps):
            z = z + omega * (dinv * (v - A @ z))
        return z
    return M


def run_product(A, b, M, restart, max_iterations, error, x0=None):
    """krylov.fgmres on CPU tensors through the shim; M as for the twin."""
    dA = DeviceCSR.from_scipy(sp.csr_matrix(A), "cpu")
    bt = torch.from_numpy(np.array(b, dtype=float).reshape(-1))
    xt = torch.zeros_like(bt) if x0 is None else torch.from_numpy(np.array(x0, dtype=float).reshape(-1))
    apply_M = None
    if M is not None:
        def apply_M(src, dst):
            dst.numpy()[:] = M(src.numpy().copy())
    r = torch.empty_like(bt)
    track, its = krylov.fgmres(shim.namespace(), dA, bt, xt, apply_M, restart=restart, max_iterations=max_iterations, error=error,
                               residual_out=r)
    np.testing.assert_allclose(r.numpy(), bt.numpy() - A @ xt.numpy(), rtol=0, atol=1e-13 * max(track[0], 1e-300))
    return xt.numpy(), track, its


def operators():
    return {"poisson": P.poisson_2d_structured(16), "stretched": P.anisotropic_poisson_2d_structured(16, 0.03, 1.0)}


# ---- 1. twin against SciPy -------------------------------------------------------------------------------------------------
def test_twin_matches_scipy_gmres():
    A, rhs = P.poisson_2d_structured(16)
    b = rhs.reshape(-1)
    _, track, its = fgmres_ref(A, b, None, restart=7, max_iterations=60, error=0.0)
    assert its == 60 and len(track) == 61
    pr = []
    spla.gmres(A, b, restart=7, rtol=1e-9, atol=0, maxiter=9, callback=pr.append, callback_type="pr_norm")
    assert len(pr) >= 60
    want = np.linalg.norm(b) * np.array(pr[:60])
    err = np.abs(np.array(track[1:]) - want).max()
    print("twin vs scipy: max |diff| / track[0] = %.3e" % (err / track[0]))
    assert err <= 1e-12 * track[0]


# ---- 2. product against twin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poisson", "stretched"])
@pytest.mark.parametrize("restart", [1, 3, 30])
@pytest.mark.parametrize("precond", ["identity", "jacobi2"])
def test_product_matches_twin(name, restart, precond):
    A, rhs = operators()[name]
    b = rhs.reshape(-1)
    M = None if precond == "identity" else jacobi_M(A, 2)
    error = 1e-8 * np.linalg.norm(b)
    xr, tr, ir = fgmres_ref(A, b, M, restart=restart, max_iterations=150, error=error)
    xp, tp, ip = run_product(A, b, M, restart, 150, error)
    assert ip == ir and len(tp) == len(tr) == ip + 1
    err = np.abs(np.array(tp) - np.array(tr)).max()
    print("%s restart %d %s: %d iterations, max history diff / track[0] = %.3e" % (name, restart, precond, ip, err / tr[0]))
    assert err <= 1e-12 * tr[0]
    assert np.linalg.norm(xp - xr) <= 1e-10 * np.linalg.norm(xr)


# ---- 3. flexibility --------------------------------------------------------------------------------------------------------
class Alternating:
    """One Jacobi sweep on even calls, three on odd ones."""

    def __init__(self, A):
        self.M = (jacobi_M(A, 1), jacobi_M(A, 3))
        self.calls = 0

    def __call__(self, v):
        self.calls += 1
        return self.M[(self.calls - 1) % 2](v)


@pytest.mark.parametrize("name", ["poisson", "stretched"])
def test_changing_preconditioner_keeps_the_estimate_true(name):
    """Cycle by cycle: a run of exactly one cycle of m steps ends on the recomputed true norm; the same steps as the first
    m of a cycle of m + 1 give the estimate that entry replaced.  x_0 + M(V y) instead of x_0 + Z y breaks the agreement."""
    A, rhs = operators()[name]
    b = rhs.reshape(-1)
    m = 5
    M = Alternating(A)
    x = np.zeros_like(b)
    t0 = None
    for cycle in range(3):
        start = M.calls
        x_new, ta, ia = run_product(A, b, M, m, m, 0.0, x0=x)
        assert ia == m and M.calls == start + m
        M.calls = start
        _, tb, ib = run_product(A, b, M, m + 1, m + 1, 0.0, x0=x)
        assert ib == m + 1
        M.calls = start + m
        t0 = ta[0] if t0 is None else t0
        print("%s cycle %d: true %.6e estimate %.6e, diff / track[0] = %.3e" % (name, cycle, ta[m], tb[m], abs(ta[m] - tb[m]) / t0))
        assert abs(ta[m] - tb[m]) <= 1e-11 * t0
        assert ta[m] < ta[0]
        x = x_new


def test_flexible_run_matches_twin_across_restarts():
    A, rhs = operators()["stretched"]
    b = rhs.reshape(-1)
    xr, tr, ir = fgmres_ref(A, b, Alternating(A), restart=4, max_iterations=30, error=0.0)
    xp, tp, ip = run_product(A, b, Alternating(A), 4, 30, 0.0)
    assert ip == ir == 30
    assert np.abs(np.array(tp) - np.array(tr)).max() <= 1e-12 * tr[0]


# ---- 4. optimality ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poisson", "stretched"])
def test_no_worse_than_the_stationary_iteration(name):
    A, rhs = operators()[name]
    b = rhs.reshape(-1)
    M = jacobi_M(A, 2)
    _, track, its = run_product(A, b, M, 12, 10, 0.0)
    assert its == 10
    x = np.zeros_like(b)
    for k in range(1, 11):
        x = x + M(b - A @ x)
        stat = np.linalg.norm(b - A @ x)
        print("%s k=%d: gmres %.6e stationary %.6e" % (name, k, track[k], stat))
        assert track[k] <= (1 + 1e-9) * stat


# ---- 5. edge cases ---------------------------------------------------------------------------------------------------------
def test_zero_rhs_and_exact_guess_take_no_iteration():
    A, rhs = P.poisson_2d_structured(8)
    b = rhs.reshape(-1)
    for run in (lambda *a, **k: run_product(*a, **k), lambda A_, b_, M, r, mi, e, x0=None: fgmres_ref(A_, b_, M, r, mi, e, x0)):
        x, track, its = run(A, np.zeros_like(b), None, 5, 50, 1e-12)
        assert its == 0 and track == [0.0] and not x.any()
        exact = spla.spsolve(A.tocsc(), b)
        x, track, its = run(A, b, None, 5, 50, 1e-10, x0=exact)
        assert its == 0 and len(track) == 1 and track[0] <= 1e-10
        np.testing.assert_array_equal(x, exact)


def test_exact_preconditioner_converges_in_one_step():
    A, rhs = P.poisson_2d_structured(8)
    b = rhs.reshape(-1)
    assert b.size == 81
    Ad = A.toarray()
    M = lambda v: np.linalg.solve(Ad, v)            # noqa: E731
    error = 1e-10 * np.linalg.norm(b)
    with np.errstate(all="raise"):
        xr, tr, ir = fgmres_ref(A, b, M, 5, 50, error)
        xp, tp, ip = run_product(A, b, M, 5, 50, error)
    assert ir == ip == 1 and len(tp) == 2
    assert tp[1] <= error and tr[1] <= error and np.isfinite(tp).all()
    np.testing.assert_allclose(xp, np.linalg.solve(Ad, b), rtol=1e-12, atol=0)


@pytest.mark.parametrize("restart,max_iterations", [(10, 4), (4, 10), (3, 1)])
def test_iteration_limit_inside_a_cycle(restart, max_iterations):
    A, rhs = P.poisson_2d_structured(16)
    b = rhs.reshape(-1)
    xr, tr, ir = fgmres_ref(A, b, jacobi_M(A, 2), restart, max_iterations, 0.0)
    xp, tp, ip = run_product(A, b, jacobi_M(A, 2), restart, max_iterations, 0.0)
    assert ip == ir == max_iterations and len(tp) == max_iterations + 1
    assert np.abs(np.array(tp) - np.array(tr)).max() <= 1e-12 * tr[0]
    # the last entry is a true norm, the cut cycle's update included
    assert abs(tp[-1] - np.linalg.norm(b - A @ xp)) <= 1e-12 * tp[0]
    assert tp[-1] < tp[0]


def test_restart_below_one_is_refused():
    A, rhs = P.poisson_2d_structured(8)
    with pytest.raises(ValueError):
        run_product(A, rhs.reshape(-1), None, 0, 10, 1e-8)


# ---- 6. keyword checks of solvers.GMRES ------------------------------------------------------------------------------------
def test_gmres_keyword_checks():
    ok = dict(restart=30, max_vectors=65, precond_smoother="Jacobi", precond_cycle_shape="V", precond_gs_sweep="forward",
              precond_line_dir="xy", precond_line_order="zebra")
    assert check_keywords(**ok) == (("forward", "forward"), {})
    assert check_keywords(**dict(ok, restart=64, precond_cycle_shape="F", precond_gs_sweep=("forward", "backward"))) == \
        (("forward", "backward"), {})
    assert check_keywords(**dict(ok, precond_cycle_shape="W", precond_gs_sweep="symmetric")) == (("symmetric", "symmetric"), {})
    assert check_keywords(**dict(ok, precond_smoother="Line")) == \
        (("forward", "forward"), {"line_dir": "xy", "line_order": "zebra", "line_band": 1})
    assert check_keywords(**dict(ok, precond_smoother="Line", precond_line_dir="y", precond_line_order="jacobi",
                                 precond_line_band=2))[1] == {"line_dir": "y", "line_order": "jacobi", "line_band": 2}
    for bad in (dict(restart=0), dict(restart=-3), dict(restart=65), dict(restart=1000), dict(restart=2.5),
                dict(precond_smoother="SOR"), dict(precond_cycle_shape="X"), dict(precond_gs_sweep="sideways"),
                dict(precond_gs_sweep=("forward",)), dict(precond_smoother="Line", precond_line_dir="z"),
                dict(precond_smoother="Line", precond_line_order="red-black")):
        with pytest.raises(ValueError):
            check_keywords(**dict(ok, **bad))


# ---- 7. the host recurrence of fgmres and block_fgmres ---------------------------------------------------------------------
def hessenberg():
    """A fixed 6 x 5 upper-Hessenberg matrix with a subdiagonal in [0.5, 1.5)."""
    rng = np.random.default_rng(3)
    H = np.triu(rng.standard_normal((6, 5)), -1)
    H[np.arange(1, 6), np.arange(5)] = 0.5 + rng.random(5)
    return H


def lstsq_bounds(Hk, y, rho):
    """(bound on |y_got - y|_2, bound on |est - rho|) against the least-squares solution y of Hk y = e_1 with residual norm rho.

    u = 2^-53.  One Givens rotation -- c and s from a hypot and two divisions, two products and a sum per rotated entry --
    moves the pair it turns by at most 10 u of its norm, a column of the k-step problem goes through at most k + 1 of them,
    and the back substitution solves (R + dR) y = g with |dR| <= k u |R| (Higham, Accuracy and Stability, Theorem 8.5): the
    computed y and g are exact for Hk + dH and e_1 + db with |dH|_F <= 11 (k + 1) u |Hk|_F, that is, with |Hk|_F <= sqrt(k) |Hk|_2,
    a relative backward error of eps_b = 11 (k + 1) sqrt(k) u in the 2-norm.  numpy.linalg.lstsq (LAPACK, backward stable)
    is allowed the same, hence the factor 2.  Theorem 20.1 there turns a backward error into
        |dy| / |y| <= kappa eps_b / (1 - kappa eps_b) (2 + (kappa + 1) rho / (|Hk|_2 |y|)),   |d rho| <= (1 + 2 kappa) eps_b |e_1|
    with kappa = cond_2(Hk): multiples of eps cond(Hk) that are computed from the reference alone."""
    k = Hk.shape[1]
    eps_b = 11.0 * (k + 1) * np.sqrt(k) * 2.0 ** -53
    kappa = np.linalg.cond(Hk)
    assert kappa * eps_b < 1e-3
    ny = np.linalg.norm(y)
    return (2.0 * kappa * eps_b / (1.0 - kappa * eps_b) * (2.0 + (kappa + 1.0) * rho / (np.linalg.norm(Hk, 2) * ny)) * ny,
            2.0 * (1.0 + 2.0 * kappa) * eps_b)


def test_arnoldi_recurrence_solves_the_least_squares_problems():
    H = hessenberg()
    ls = krylov.Arnoldi(1.0)
    assert ls.solution() == []
    for j in range(5):
        est = ls.step(H[:j + 1, j].tolist(), float(H[j + 1, j]))
        Hk, e1 = H[:j + 2, :j + 1], np.eye(j + 2)[0]
        want = np.linalg.lstsq(Hk, e1, rcond=None)[0]
        rho = np.linalg.norm(e1 - Hk @ want)
        got = np.array(ls.solution())
        by, br = lstsq_bounds(Hk, want, rho)
        print("step %d: cond %.2f, |y - lstsq| %.2e (bound %.2e), |est - rho| %.2e (bound %.2e)"
              % (j, np.linalg.cond(Hk), np.linalg.norm(got - want), by, abs(est - rho), br))
        assert got.shape == (j + 1,) and len(ls.g) == j + 2 and len(ls.cs) == len(ls.sn) == len(ls.R) == j + 1
        assert 0.0 < rho < 1.0 and est == abs(ls.g[j + 1])
        assert np.linalg.norm(got - want) <= by
        assert abs(est - rho) <= br


def test_arnoldi_recurrence_breakdowns():
    # |w| == 0 at the last step: the Krylov space is invariant, the square system is solved exactly
    H = hessenberg()
    ls = krylov.Arnoldi(1.0)
    for j in range(4):
        assert ls.step(H[:j + 1, j].tolist(), float(H[j + 1, j])) > 0.0
    assert ls.step(H[:5, 4].tolist(), 0.0) == 0.0 and ls.sn[4] == 0.0
    want = np.linalg.solve(H[:5, :5], np.eye(5)[0])
    by, _ = lstsq_bounds(H[:5, :5], want, 0.0)
    assert np.linalg.norm(np.array(ls.solution()) - want) <= by
    # a column that is zero after the earlier rotations, with |w| == 0: the (1, 0) rotation, and y = 0 at the zero pivot
    ls = krylov.Arnoldi(1.0)
    assert ls.step([2.0], 0.0) == 0.0
    assert ls.step([3.0, 0.0], 0.0) == 0.0
    assert (ls.cs, ls.sn) == ([1.0, 1.0], [0.0, 0.0]) and ls.R[1] == [3.0, 0.0]
    assert ls.solution() == [0.5, 0.0]
    ls = krylov.Arnoldi(7.0)
    assert ls.step([0.0], 0.0) == 0.0 and ls.solution() == [0.0] and ls.g[0] == 7.0
