"""solvers.GMRES on the device (-m gpu): against the NumPy twin (tests/krylov_ref.py) driven with the same multigrid cycle,
against the stationary iteration of that cycle, against SciPy's GMRES without a preconditioner, on the operators and the
cycles CG cannot take, the solver-class conventions, and CG unchanged by the preconditioner helper it now shares."""
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from conftest import coo_from, load_golden                         # noqa: E402
from krylov_ref import fgmres_ref                                  # noqa: E402
from learnmultigrid_amd import ops, problems as P                  # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy                 # noqa: E402
from learnmultigrid_amd.solvers import CG, GMRES                   # noqa: E402
from support import DEV                                            # noqa: E402


def cycle_operator(H, smoother, steps, omega, shape="V", gs_sweep=("forward", "forward")):
    """M(r): one cycle of H on the right-hand side r from a zero guess, the way the MG-PCG tests apply it."""
    fine = H.levels[0]

    def M(r):
        fine.b.copy_(torch.from_numpy(np.ascontiguousarray(r)).to(DEV))
        H.cycle(smoother, steps, omega, x_is_zero=True, gs_sweep=gs_sweep, shape=shape)
        return fine.x.cpu().numpy().copy()
    return M


def stationary_count(A, b, M, error, limit):
    """Cycles of x <- x + M(b - A x) from zero until |b - A x| <= error."""
    x = np.zeros_like(b)
    for k in range(1, limit + 1):
        x = x + M(b - A @ x)
        if np.linalg.norm(b - A @ x) <= error:
            return k
    return limit + 1


# ---- 11. stretched operator ------------------------------------------------------------------------------------------------
def test_stretched_operator_against_twin_and_stationary_cycle():
    """Prototype figures of the design: 138 stationary damped-Jacobi V(2,2) cycles, 29 GMRES(10) iterations."""
    A, rhs = P.anisotropic_poisson_2d_structured(64, 0.03, 1.0)
    b = rhs.reshape(-1)
    H = Hierarchy(A, P.geometric_hierarchy_2d(65, 4), DEV)
    error = 1e-8 * np.linalg.norm(b)
    M = cycle_operator(H, "Jacobi", 2, 0.8)
    stat = stationary_count(A, b, M, error, 400)
    g = GMRES(A, rhs.copy())
    g.solve(max_iterations=200, error=error, restart=10, preconditioner=H, precond_smoother="Jacobi", precond_steps=2,
            precond_omega=0.8)
    its, track = g.get_iterations(), g.get_track_res().ravel()
    xr, tr, ir = fgmres_ref(A, b, M, restart=10, max_iterations=200, error=error)
    diff = np.abs(track - np.array(tr)).max() if len(tr) == len(track) else float("nan")
    true = np.linalg.norm(b - A @ g.get_solution().ravel())
    print("stationary %d cycles, GMRES %d iterations, twin %d; history diff / track[0] = %.3e; |final - true| / track[0] = %.3e"
          % (stat, its, ir, diff / track[0], abs(track[-1] - true) / track[0]))
    assert stat <= 400 and its > 10                       # (crosses a restart)
    assert 3 * its <= stat
    assert its == ir and len(track) == len(tr)
    assert diff <= 1e-12 * track[0]
    assert track[-1] <= error
    assert abs(track[-1] - true) <= 1e-11 * track[0]


# ---- 12. the operators and cycles CG cannot take ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def poisson65():
    A, rhs = P.poisson_2d_structured(64)
    assert abs(A - A.T).max() > 0                         # identity boundary rows, columns untouched
    return A, rhs, spla.spsolve(A.tocsc(), rhs.reshape(-1))


@pytest.mark.parametrize("kw", [
    dict(precond_smoother="GaussSeidel", precond_steps=1),
    dict(precond_smoother="Jacobi", precond_cycle_shape="F"),
    dict(precond_smoother="Chebyshev", precond_steps=2),
    dict(precond_cycle_shape="W"),
], ids=["gs-forward-forward", "jacobi-F", "chebyshev", "W"])
def test_unsymmetric_operator_and_cycles(poisson65, kw):
    A, rhs, x_ref = poisson65
    b = rhs.reshape(-1)
    H = Hierarchy(A, P.geometric_hierarchy_2d(65, 4), DEV)
    smoother = kw.get("precond_smoother", "Jacobi")
    steps = kw.get("precond_steps", 2)
    M = cycle_operator(H, smoother, steps, 0.8 if smoother == "Jacobi" else 1.0, kw.get("precond_cycle_shape", "V"))
    stat = stationary_count(A, b, M, 1e-10, 200)
    g = GMRES(A, rhs.copy())
    g.solve(max_iterations=200, error=1e-10, restart=30, preconditioner=H, **kw)
    x = g.get_solution().ravel()
    print("%s: GMRES %d iterations, stationary %d, final %.3e" % (kw, g.get_iterations(), stat, g.get_residual()))
    assert g.get_residual() <= 1e-10 and g.get_track_res()[-1, 0] == g.get_residual()
    assert g.get_iterations() <= stat <= 200
    assert np.linalg.norm(x - x_ref) <= 1e-8 * np.linalg.norm(x_ref)


# ---- 13. plain GMRES against SciPy -----------------------------------------------------------------------------------------
def test_plain_gmres_matches_scipy():
    A, rhs = P.poisson_2d_structured(16)
    b = rhs.reshape(-1)
    g = GMRES(A, rhs.copy())
    g.solve(max_iterations=60, error=0.0, restart=7)
    track = g.get_track_res().ravel()
    assert g.get_iterations() == 60 and track.shape == (61,)
    pr = []
    spla.gmres(A, b, restart=7, rtol=1e-9, atol=0, maxiter=9, callback=pr.append, callback_type="pr_norm")
    want = np.linalg.norm(b) * np.array(pr[:60])
    err = np.abs(track[1:] - want).max()
    print("device vs scipy: max |diff| / track[0] = %.3e" % (err / track[0]))
    assert abs(track[0] - np.linalg.norm(b)) <= 1e-14 * track[0]
    assert err <= 1e-12 * track[0]


# ---- 14. solver-class conventions ------------------------------------------------------------------------------------------
def test_solver_class_conventions():
    A, rhs = P.poisson_2d_structured(16)
    n = A.shape[0]
    H = Hierarchy(A, P.geometric_hierarchy_2d(17, 3), DEV)
    g = GMRES(A, rhs.copy())
    assert g.label == "GMRES" and g.get_iterations() == 0
    g.solve(error=1e-10, restart=5, preconditioner=H)
    first = g.get_track_res().copy()
    assert first.shape == (g.get_iterations() + 1, 1) and g.get_iterations() >= 1
    assert g.get_solution().shape == (n, 1) and g.get_residual_vector().shape == (n, 1)
    assert g.get_residual() == first[-1, 0] <= 1e-10
    np.testing.assert_allclose(g.get_residual_vector(), rhs - A @ g.get_solution(), rtol=0, atol=1e-13)
    # a supplied initial guess is used and not mutated
    guess = np.linspace(0.0, 1.0, n)
    keep = guess.copy()
    g.solve(error=1e-10, restart=5, preconditioner=H, initial_guess=guess)
    assert np.array_equal(guess, keep)
    assert abs(g.get_track_res()[0, 0] - np.linalg.norm(rhs.ravel() - A @ keep)) <= 1e-12 * g.get_track_res()[0, 0]
    assert g.get_track_res().shape == (g.get_iterations() + 1, 1) and g.get_residual() <= 1e-10
    # a second solve on the same object repeats the first
    g.solve(error=1e-10, restart=5, preconditioner=H)
    assert np.array_equal(g.get_track_res(), first)
    # an iteration limit inside a cycle: the last entry is still a true norm
    g.solve(max_iterations=3, error=0.0, restart=5)
    assert g.get_iterations() == 3 and g.get_track_res().shape == (4, 1)
    assert abs(g.get_residual() - np.linalg.norm(rhs - A @ g.get_solution())) <= 1e-12 * g.get_track_res()[0, 0]
    for bad in (dict(restart=0), dict(restart=ops.krylov_max_vectors()), dict(precond_smoother="SOR"),
                dict(precond_cycle_shape="X"), dict(precond_gs_sweep="sideways")):
        with pytest.raises(ValueError):
            g.solve(preconditioner=H, **bad)
    # the largest basis the solver takes, one whole cycle of it
    A2, rhs2 = P.anisotropic_poisson_2d_structured(16, 0.03, 1.0)
    g2 = GMRES(A2, rhs2.copy())
    g2.solve(max_iterations=ops.krylov_max_vectors() - 1, error=0.0, restart=ops.krylov_max_vectors() - 1)
    assert g2.get_iterations() == ops.krylov_max_vectors() - 1
    assert abs(g2.get_residual() - np.linalg.norm(rhs2 - A2 @ g2.get_solution())) <= 1e-12 * g2.get_track_res()[0, 0]
    assert g2.get_residual() < 1e-3 * g2.get_track_res()[0, 0]


# ---- 15. CG is unchanged by the shared helper ------------------------------------------------------------------------------
def test_g6_cg_still_matches_its_golden_history():
    g = load_golden("g6_cg_ne64")
    c = CG(coo_from(g, "A"), g["rhs"])
    c.solve(max_iterations=200, error=1e-10)
    assert c.get_iterations() == int(g["iterations"])
    assert c.get_track_res().shape == g["track"].shape
    np.testing.assert_allclose(c.get_track_res()[:20], g["track"][:20], rtol=1e-8)
    np.testing.assert_allclose(c.get_solution(), g["solution"], rtol=1e-9, atol=1e-12)


def inline_make_apply(H, precond_smoother, precond_steps, precond_omega, precond_cycle_shape, gs_sweep, options):
    """What CG.solve did inline before the preconditioner moved to solvers/_precond.py, kept here for the comparison."""
    precond_line_dir, precond_line_order = options.get("line_dir"), options.get("line_order")
    assert gs_sweep == ("forward", "backward")
    if H is not None and precond_smoother == "Chebyshev":
        H.prepare_smoother("Chebyshev")
    if H is not None and precond_smoother == "Line":
        H.prepare_smoother("Line", line_dir=precond_line_dir, line_order=precond_line_order)

    def apply_M(src, dst):
        if H is None:
            ops.copy(src, dst)
            return
        fine = H.levels[0]
        ops.copy(src, fine.b)
        if precond_smoother == "GaussSeidel":
            H.cycle("GaussSeidel", precond_steps, 1.0, x_is_zero=True, gs_sweep=("forward", "backward"),
                    shape=precond_cycle_shape)
        elif precond_smoother == "Chebyshev":
            H.cycle("Chebyshev", precond_steps, 1.0, x_is_zero=True, shape=precond_cycle_shape)
        elif precond_smoother == "Line":
            H.cycle("Line", precond_steps, precond_omega, x_is_zero=True, shape=precond_cycle_shape)
        else:
            H.cycle("Jacobi", precond_steps, precond_omega, x_is_zero=True, shape=precond_cycle_shape)
        ops.copy(fine.x, dst)
    return apply_M


@pytest.mark.parametrize("kw", [
    dict(precond_smoother="Jacobi"),
    dict(precond_smoother="GaussSeidel", precond_steps=1),
    dict(precond_smoother="Chebyshev", precond_cycle_shape="W"),
    dict(precond_smoother="Line", precond_omega=1.0, precond_steps=1),
], ids=["Jacobi", "GaussSeidel", "Chebyshev", "Line"])
def test_mg_pcg_history_is_the_inline_one(monkeypatch, kw):
    m = 64
    A, rhs = P.poisson_2d_structured(m)
    s = m + 1
    idx = np.arange(s * s)
    inter = ((idx % s) > 0) & ((idx % s) < m) & ((idx // s) > 0) & ((idx // s) < m)
    keep = sp.diags(inter.astype(float))
    As = sp.csr_matrix(keep @ A @ keep + sp.diags((~inter).astype(float)))
    tracks = []
    for inline in (False, True):
        with monkeypatch.context() as mp:
            if inline:
                mp.setattr(sys.modules["learnmultigrid_amd.solvers.CG"], "make_apply", inline_make_apply)
            H = Hierarchy(As, P.geometric_hierarchy_2d(s, 4), DEV)
            c = CG(As, rhs.copy())
            c.solve(max_iterations=50, error=1e-10, preconditioner=H, **kw)
            assert 1 <= c.get_iterations() < 50
            tracks.append((c.get_track_res().copy(), c.get_solution().copy()))
    assert np.array_equal(tracks[0][0], tracks[1][0]) and np.array_equal(tracks[0][1], tracks[1][1])
