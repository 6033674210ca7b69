"""The classical AMG setup on an MI355X (-m gpu): learnmultigrid_amd/amg.py and csrc/amg.hip against the plain-Python twin of
their rules (tests/amg_ref.py) -- every integer equal, every value bit for bit --, on the case matrices and edge shapes of
tests/amg_cases.py; then whole hierarchies through solvers.ClassicalAMG against the oracle's cycle on the twin's transfers.

Each whole-hierarchy test prints its largest relative deviation from the oracle's history before it asserts."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import amg_cases as C                                              # noqa: E402
import amg_ref as R                                                # noqa: E402
from learnmultigrid_amd import amg, ops, problems as P             # noqa: E402
from learnmultigrid_amd.hierarchy import Hierarchy                 # noqa: E402
from learnmultigrid_amd.solvers import GMRES, ClassicalAMG, HierarchyMG   # noqa: E402
from support import DEV, dev                                       # noqa: E402

CASES = sorted(C.case_matrices())
RTOL, FLOOR = 1e-10, 1e-14                                          # the project's standing bound for cycles (deviation below)


def host(M):
    """A DeviceCSR as (shape, rowptr, colidx, vals) on the host."""
    return M.shape, M.rowptr.cpu().numpy(), M.colidx.cpu().numpy(), M.vals.cpu().numpy()


def assert_csr_equal(got, want, what):
    """The DeviceCSR `got` is the SciPy CSR `want`: shape, integers, and the values bit for bit."""
    shape, rp, ci, va = host(got)
    assert shape == want.shape, what
    assert np.array_equal(rp, want.indptr) and np.array_equal(ci, want.indices), what
    assert np.array_equal(va.view(np.int64), want.data.view(np.int64)), what


def assert_same_tensors(a, b, what):
    for x, y in zip(a, b):
        assert torch.equal(x, y), what


# ---- stage parity against the twin, edge shapes included -----------------------------------------------------------------------
@pytest.mark.parametrize("split", ["pmis", "greedy"])
@pytest.mark.parametrize("name", CASES)
def test_stages_are_the_twins_integers_and_bits(name, split):
    A, theta = C.case_matrices()[name]
    n = A.shape[0]
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    # strength
    S = R.strength(A, theta)
    dS = amg.strength_device(dA, theta)
    assert_csr_equal(dS, S, "S")
    dS2 = amg.strength_device(dA, theta)
    assert torch.equal(dS.rowptr, dS2.rowptr) and torch.equal(dS.colidx, dS2.colidx)
    # split
    state, rank, n_c, rounds = R.split_of(S, split)
    d_state, d_rank, d_nc, d_rounds = amg.split_device(dS, split)
    assert (d_nc, d_rounds) == (n_c, rounds)
    assert np.array_equal(d_state.cpu().numpy(), state) and np.array_equal(d_rank.cpu().numpy(), rank)
    again = amg.split_device(dS, split)
    assert torch.equal(again[0], d_state) and torch.equal(again[1], d_rank) and again[2:] == (d_nc, d_rounds)
    if split == "greedy":
        assert np.array_equal(state == R.COARSE, ops.host_greedy_cf(S) != 0)
    if n_c in (0, n):
        assert amg.transfer_device(dA, theta, split)[0] is None
        return
    # direct interpolation
    P0 = R.direct_interpolation(A, S, state, rank)
    dP0 = amg.direct_interpolation_device(dA, dS, d_state, d_rank)
    assert_csr_equal(dP0, P0, "direct P")
    assert_same_tensors(host_tensors(amg.direct_interpolation_device(dA, dS, d_state, d_rank)), host_tensors(dP0), "direct twice")
    # the Jacobi step, with the defaults and with another damping and truncation
    for omega, trunc in ((1.0, 0.2), (0.7, 0.0), (1.0, 1.0)):
        P1 = R.smooth_interpolation(A, P0, state, rank, omega, trunc)
        dP1 = amg.smooth_interpolation_device(dA, dP0, d_state, d_rank, omega, trunc)
        assert_csr_equal(dP1, P1, "smoothed P %s" % ((omega, trunc),))
        assert_same_tensors(host_tensors(amg.smooth_interpolation_device(dA, dP0, d_state, d_rank, omega, trunc)),
                            host_tensors(dP1), "smoothed twice")
    # a second step on the first one's result (interp_sweeps = 2): rows of P that are no subset of the direct pattern
    P1 = R.smooth_interpolation(A, P0, state, rank)
    dP1 = amg.smooth_interpolation_device(dA, dP0, d_state, d_rank)
    assert_csr_equal(amg.smooth_interpolation_device(dA, dP1, d_state, d_rank), R.smooth_interpolation(A, P1, state, rank), "second step")


def host_tensors(M):
    return M.rowptr, M.colidx, M.vals


def test_a_pivot_that_is_not_finite_is_refused_with_its_row():
    """d_i = a_ii + (the couplings of a_ii's sign) cannot be 0 with finite entries (the lumped couplings carry the diagonal's
    sign); the refusal that can be reached is the d_i that overflows (amg_cases.overflow_row)."""
    A, state, row = C.overflow_row()
    dA = ops.DeviceCSR.from_scipy(A, DEV)
    dS = amg.strength_device(dA)
    assert_csr_equal(dS, R.strength(A), "S")
    rank = R.ranks(state)[0]
    with pytest.raises(amg.Refused) as e:
        amg.direct_interpolation_device(dA, dS, dev(state), dev(rank))
    assert (e.value.rule, e.value.row) == ("pivot", row)
    with pytest.raises(R.Refused):
        R.direct_interpolation(A, R.strength(A), state, rank)


def test_keywords_are_checked_on_the_host():
    dA = ops.DeviceCSR.from_scipy(C.chain(5), DEV)
    for kw in (dict(theta=-0.1), dict(theta=1.5), dict(interp_trunc=2.0), dict(interp_omega=float("nan")), dict(split="rs"),
               dict(max_levels=0), dict(interp_sweeps=-1)):
        with pytest.raises(ValueError):
            amg.classical_hierarchy(dA, DEV, max_coarse=2, **kw)


# ---- whole hierarchies --------------------------------------------------------------------------------------------------------
SOLVE = dict(smoother="Jacobi", smooth_steps=2, omega=0.8, smoother_semantics="as_named")


def deviation(got, want, largest):
    """The largest |got - want| in units of the project's standing bound for residual histories (tests/test_solvers_gpu.py,
    __graft_entry__.smoke): 1e-10 relative, with a floor of 1e-14 of the run's largest entry -- here `largest` = ||b||, the
    residual the run starts from.  The floor is what the histories of these tests need: they run down to 1e-8 ||b||, where
    the rounding of the iterate alone (eps |A| |x|, some 1e-17 here, 1e-15 ||b||) is 1e-7 of the residual.  Measured on the
    five problems: at most 4.6e-7 relative on the last entries, and a constant 1e-17 in absolute terms, whatever
    coarse_refine is (the coarsest solve leaves a residual of 6e-16)."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / (RTOL * np.abs(want) + FLOOR * largest)))


def solver_for(name, **kw):
    A, b = C.problems()[name]
    return ClassicalAMG(A, b.reshape(-1, 1).copy(), **dict(C.AMG_KW, **kw)), A, b


@pytest.mark.parametrize("name", sorted(C.problems()))
def test_classical_amg_solve_matches_the_oracle_on_the_twins_transfers(name):
    """V(2,2) damped Jacobi (0.8), max_coarse=100, to 1e-8 ||b||: the level sizes of the twin, the oracle's residual history
    within 1e-10 relative, at most 30 cycles (the twin's counts: tests/test_amg_cpu.py)."""
    mg, A, b = solver_for(name)
    Ps, As, infos = C.twin_hierarchy(name)
    want = C.oracle_history(A, b, Ps)
    mg.solve(max_iterations=C.CAP + 1, error=C.TARGET * np.linalg.norm(b), **SOLVE)
    assert mg.level_dims == [M.shape[0] for M in As]
    got = mg.get_track_res().ravel()
    assert got[0] == np.sqrt(A.shape[0])                           # (the reference's first entry)
    print("%s: levels %s, %d cycles, deviation %.3f of the bound" % (name, mg.level_dims, got.size - 1, deviation(got[1:], want[1:], want[0])))
    assert deviation(got[1:], want[1:], want[0]) <= 1.0
    assert got.size - 1 == C.cycles_needed(want) <= C.CAP and got[-1] <= C.TARGET * np.linalg.norm(b)
    info = mg.hierarchy_info()
    assert [(d["n"], d["nnz"]) for d in info["levels"]] == [(M.shape[0], M.nnz) for M in As]
    assert [(d["n_c"], d["rounds"]) for d in info["levels"][:len(infos)]] == [(d["n_c"], d["rounds"]) for d in infos]
    assert info["operator_complexity"] == sum(M.nnz for M in As) / As[0].nnz
    assert info["grid_complexity"] == sum(M.shape[0] for M in As) / As[0].shape[0]
    # the transfers stayed on the device and are the twin's, bit for bit
    for lev, Pt in zip(mg._hier.levels, Ps):
        assert_csr_equal(lev.P, Pt, "P")


def test_levels_is_an_upper_limit_and_the_cycles_are_callable():
    mg, A, b = solver_for("jittered")
    Ps = C.twin_hierarchy("jittered")[0]
    mg.solve(levels=2, max_iterations=3, error=0.0, **SOLVE)
    assert mg.level_dims == [A.shape[0], Ps[0].shape[1]]
    want = C.oracle_history(A, b, Ps[:1], cap=2, target=0.0)
    print("two levels: deviation %.3f of the bound" % deviation(mg.get_track_res().ravel()[1:], want[1:3], want[0]))
    assert deviation(mg.get_track_res().ravel()[1:], want[1:3], want[0]) <= 1.0
    x0 = np.zeros((A.shape[0], 1))
    outs = [f(mg.get_matrix(), x0.copy(), b.reshape(-1, 1), "Jacobi", 2, 0.0, 10, omega=0.8, smoother_semantics="as_named")
            for f in (mg.v_cycle, mg.w_cycle, mg.f_cycle)]
    res = [np.linalg.norm(b.ravel() - A @ o.ravel()) for o in outs]
    first = C.oracle_history(A, b, Ps, cap=1, target=0.0)[1]
    print("one V, W, F cycle:", res, "oracle's V:", first)
    assert abs(res[0] - first) <= RTOL * first + FLOOR * np.linalg.norm(b)     # the V-cycle is the first cycle of the whole solve
    assert max(res) < np.linalg.norm(b)


def test_gauss_seidel_as_shipped():
    mg, A, b = solver_for("jittered")
    want = C.oracle_history(A, b, C.twin_hierarchy("jittered")[0], smoother="GaussSeidel", steps=2)
    mg.solve(smooth_steps=2, max_iterations=C.CAP + 1, error=C.TARGET * np.linalg.norm(b))
    got = mg.get_track_res().ravel()
    print("Gauss-Seidel: %d cycles, deviation %.3f of the bound" % (got.size - 1, deviation(got[1:], want[1:], want[0])))
    assert deviation(got[1:], want[1:], want[0]) <= 1.0
    assert got.size - 1 == C.cycles_needed(want) <= C.CAP


def test_w_cycle_solve_many_and_gmres_on_one_hierarchy():
    mg, A, b = solver_for("jittered")
    nb = np.linalg.norm(b)
    want = C.oracle_history(A, b, C.twin_hierarchy("jittered")[0])
    v_cycles = C.cycles_needed(want)
    mg.solve(max_iterations=C.CAP + 1, error=C.TARGET * nb, cycle_shape="W", **SOLVE)
    w = mg.get_track_res().ravel()
    print("W: %d cycles against %d V" % (w.size - 1, v_cycles))
    assert w[-1] <= C.TARGET * nb and w.size - 1 <= v_cycles and np.all(w[2:] < w[1:-1])
    # four columns: the problem's own and three scalings by powers of two, whose histories are the same numbers scaled
    scale = np.array([1.0, 2.0, -0.5, 4.0])
    X, track = mg.solve_many(b.reshape(-1, 1) * scale, smooth_steps=2, omega=0.8, max_iterations=C.CAP + 1, error=C.TARGET * nb * 0.5)
    for j in range(4):
        col = track[:, j]
        col = col[~np.isnan(col)]
        m = min(col.size, len(want))
        ref = np.abs(scale[j]) * np.array(want[:m])
        print("solve_many column %d: deviation %.3f of the bound" % (j, deviation(col[:m], ref, ref[0])))
        assert deviation(col[:m], ref, ref[0]) <= 1.0
        assert np.linalg.norm(b.ravel() * scale[j] - A @ X[:, j]) <= C.TARGET * nb * abs(scale[j])
    # the same hierarchy as a preconditioner
    H = mg.setup()
    assert isinstance(H, Hierarchy) and H.sizes == mg.level_dims
    g = GMRES(A, b.reshape(-1, 1).copy())
    g.solve(max_iterations=60, error=C.TARGET * nb, preconditioner=H, precond_steps=2, precond_omega=0.8)
    print("GMRES: %d iterations against %d cycles" % (g.get_iterations(), v_cycles))
    assert g.get_residual() <= C.TARGET * nb and g.get_iterations() < v_cycles


def test_anisotropic_problem_against_the_geometric_hierarchy():
    """0.01 u_xx + u_yy under V(2,2) damped Jacobi.  On the oracle (tests/test_amg_cpu.py): the geometric hierarchy has not
    reached 1e-8 ||b|| after 30 cycles, the algebraic one has after 19.  The same on the device."""
    mg, A, b = solver_for("anisotropic")
    nb = np.linalg.norm(b)
    geo = HierarchyMG(A, b.reshape(-1, 1).copy(), P.geometric_hierarchy_2d(33, 3))
    geo.solve(levels=3, max_iterations=C.CAP + 1, error=C.TARGET * nb, **SOLVE)
    mg.solve(max_iterations=C.CAP + 1, error=C.TARGET * nb, **SOLVE)
    print("geometric after 30 cycles: %.3e ||b||; algebraic: %d cycles" % (geo.get_residual() / nb, mg.get_iterations() - 1))
    assert geo.get_iterations() == C.CAP + 1 and geo.get_residual() > C.TARGET * nb
    assert mg.get_residual() <= C.TARGET * nb and mg.get_iterations() - 1 <= C.CAP


def test_a_matrix_without_a_coarse_level_is_refused_by_the_solver():
    A = C.case_matrices()["diagonal"][0]
    H = amg.classical_hierarchy(A, DEV, max_coarse=2)
    assert H.sizes == [5] and H.amg_info[0]["n_c"] == 0
    with pytest.raises(ValueError, match="no coarse level"):
        ClassicalAMG(A, np.ones((5, 1)), max_coarse=2).solve()
